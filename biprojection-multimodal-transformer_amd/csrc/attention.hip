// Fused crossmodal / self attention for BPMulT on gfx950: forward, dQ, dK/dV.
//
// Semantics (reference multihead_attention.py:86-130, transformer.py:209-216):
//   S = Qs K^T  (Qs already carries the dh^-0.5 scale, applied by the Q-projection epilogue)
//   key j visible to query i  iff  j - i < mask_off   (mask_off = 1 + |S-T|, or "infinite" without attn_mask)
//   P = softmax_fp32(S) over visible keys;  Pd = dropout(P);  O = Pd V
// No key-padding mask: zero-padded key rows take part.
// Two further visibility rules are separate instantiations of the same block bodies (compile-time flags; the kernels
// above never see them): the per-key byte mask of the *_kmask entries (KM) and the arbitrary additive fp32 [T, S] mask of
// the *_amask entries (AM: the reference's attn_mask argument as a tensor, multihead_attention.py:113-115), one image for
// all heads, or one per head through the *_hmask entries (a learned bias; its gradient is attn_dbias_kernel below).
// The [T,S] score matrix never touches HBM: forward keeps a running (max, sum)
// per query and stores only LSE = max + ln(sum); backward recomputes P from
// Q, K and LSE.
//
// Layouts (HBM):  Q [B,H,T,dhp], K/V [B,H,S,dhp], dO [B,H,T,dhp]  -- CT,
// head-major, dhp = head_dim padded to 32 with zeros, written by the
// projection GEMM epilogues.  O, dQ, dK, dV are row-major [(t*B+b), ld]
// with column h*dh + c: the operand layout of the out-proj / in-proj GEMMs.
//
// MFMA orientation ("key on the rows" for forward and dQ, "key on the lane"
// for dK/dV; cdna_hip_programming.md Appendix B): the score tile is produced
// with the reduction index of the NEXT product on its register rows, so P / dS
// feed the second MFMA straight from the accumulator registers (pack_rows)
// and the other operand is read transposed from the LDS image (read_tr).
//   forward / dQ : S^T = K Qs^T   -> rows = keys, lane = query
//                  O^T  += V^T  Pd^T      dQ^T += K^T dS^T
//   dK/dV        : S   = Qs K^T   -> rows = queries, lane = key
//                  dV^T += dO^T Pd        dK^T += Qs^T dS
// One wave owns 16 queries (or 16 keys); a 256-thread workgroup owns 64.
//
// At head_dim 25 the kernels are VALU-bound (16 exponentials per 8 MFMAs), so
// the element loops are kept to a handful of instructions: visibility is one
// compare against a per-lane limit and is skipped altogether on tiles that a
// wave-uniform test proves fully visible; dropout hashing runs only when
// enabled; exponentials are raw v_exp_f32.
#include <type_traits>

#include "bpm_common.h"
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
// keep their argument layout (and their code: the block bodies below take the mask as a compile-time switch).
struct AMask { const uint8_t* mask; int ldm; };
struct AGroupK {
    AGroup g;
    AMask m[BPM_MAX_GROUP];
};
static_assert(sizeof(AGroupK) <= 4096, "kernel arguments are limited to 4 KiB");

// Additive mask of the *_amask entries (the reference's attn_mask argument, multihead_attention.py:113-115): fp32 [T, ldm],
// added to the score of (query i, key j) in every head of the problem; -inf hides the pair.  The forward and dQ kernels
// hold one query per lane and 4 consecutive keys per register group: they read `mask` rows as float4.  The dK / dV and
// maps kernels hold one key per lane and 4 consecutive queries per register group: they read the TRANSPOSE [S, ldt] the
// caller supplies, again as float4 (reading `mask` down a column would be 16 scalar loads per lane and tile).  One
// descriptor per kernel: m / ld are (mask, ldm) or (maskT, ldt).  A third argument block beside AGroup / AGroupK: without
// AM none of this is compiled.  hs: elements between the images of consecutive heads (head h of every sample reads
// m + h * hs); 0: one image for all heads.
struct AAdd { const float* m; int ld; int hs; };
struct AGroupA {
    AGroup g;
    AAdd m[BPM_MAX_GROUP];
};
static_assert(sizeof(AGroupA) <= 4096, "kernel arguments are limited to 4 KiB");

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
// forward
// ---------------------------------------------------------------------------
// KM: with a per-key mask (AMask).  The tile's KT mask bytes are fetched one tile ahead by the first KT threads (never at
// j >= S: those keys are hidden without a load), pass through KT bytes of LDS behind the K / V images as 0 / 1, and every
// lane reads the four words that cover its 16 keys.  A hidden key's score becomes -inf before the maximum, like a key
// beyond the mask_off limit; a tile without any visible key is skipped.  Without KM none of this is compiled.
// AM: with an additive mask (AAdd).  A lane's 16 keys of a tile are four groups of 4 consecutive columns of its query's
// mask row: four float4 loads, issued before the score MFMAs and added to the scores before the visibility selects (so
// whatever sits in columns >= S, which the limit hides, never survives).  Never read at q >= T or at a group that starts
// at j >= S.  No tile is skipped; the running maximum takes the KM guard.
template <typename CT, int DHP, bool KM, bool AM = false>
BPM_DEV void attn_fwd_block(const AProb& P, const DropCfg& drop, char* smem, const int bh, const int qb, const AMask km,
                            const AAdd am = AAdd{nullptr, 0, 0}) {
    typedef Cfg<CT, DHP> C;
    typedef typename Tr<CT>::frag frag;
    char* kimg = smem;
    char* vimg = smem + KT * C::STRIDE;
    uint8_t* smask = (uint8_t*)(smem + 2 * KT * C::STRIDE);    // KM only

    const int b = bh / P.H, h = bh % P.H;
    int tid_ = threadIdx.x;
    asm volatile("" : "+v"(tid_));                 // per-lane values are re-derived in each pass of the block-pair loop, not kept live across it
    const int tid = tid_, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int q0 = qb * 64 + wave * 16;               // wave-uniform first query
    const int q = q0 + c;                             // this lane's query
    const char* Qh = P.Q + (size_t)bh * P.T * C::ROWB;
    const char* Kh = P.K + (size_t)bh * P.S * C::ROWB;
    const char* Vh = P.V + (size_t)bh * P.S * C::ROWB;

    frag qf[C::NKS];
#pragma unroll
    for (int s = 0; s < C::NKS; ++s) qf[s] = load_frag<CT, DHP>(Qh, q, P.T, s, g);

    f32x4 o[C::ND];
#pragma unroll
    for (int n = 0; n < C::ND; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    const int q_hi = min(P.T, qb * 64 + 64) - 1;
    const int jend = min(P.S, P.qpos0 + q_hi * P.qstride + P.mask_off);      // one past the last key any query of this block sees (mask_off < 2^30)
    const int ntile = (jend + KT - 1) / KT;
    const int lim = min(P.S, P.qpos0 + q * P.qstride + P.mask_off);          // this lane sees keys j < lim
    const int lim_min = min(P.S, P.qpos0 + q0 * P.qstride + P.mask_off);     // every lane of the wave sees keys j < lim_min
    const bool dropping = drop.thresh != 0;
    const uint32_t drow = ((uint32_t)bh * (uint32_t)P.T + (uint32_t)q) * (uint32_t)P.S;
    const bool pair_ok = (P.S & 3) == 0;               // row starts are multiples of 4: keys (4m .. 4m+3) are one hash quad

    RowStage<CT, DHP, KT> kst, vst;
    uint32_t n_vis = 0;                                // KM, threads < KT: next tile's visibility of key kt * KT + tid
    auto stage_mask = [&](int kt) {
        const int jm = kt * KT + tid;
        n_vis = 0;
        if (tid < KT && jm < P.S) n_vis = km.mask[(size_t)b * km.ldm + jm] != 0;
    };
    if (ntile > 0) {
        kst.load(Kh, 0, P.S, tid); vst.load(Vh, 0, P.S, tid);
        if constexpr (KM) stage_mask(0);
    }
    const float* arow = nullptr;                       // AM: this lane's mask row
    if constexpr (AM) arow = am.m + (size_t)h * am.hs + (size_t)min(q, P.T - 1) * am.ld;
#pragma unroll 1
    for (int kt = 0; kt < ntile; ++kt) {
        __syncthreads();
        kst.store(kimg, tid);
        vst.store(vimg, tid);
        if constexpr (KM) { if (tid < KT) smask[tid] = (uint8_t)n_vis; }
        __syncthreads();
        if (kt + 1 < ntile) {
            kst.load(Kh, (kt + 1) * KT, P.S, tid); vst.load(Vh, (kt + 1) * KT, P.S, tid);
            if constexpr (KM) stage_mask(kt + 1);
        }
        f32x4 am4[4];                                  // AM: mask of keys kt * KT + 16n + 4g + (0..3)
        if constexpr (AM) {
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int jc = kt * KT + 16 * n + 4 * g;        // jc % 4 == 0 and ldm % 4 == 0: jc < S implies jc + 3 < ldm
                am4[n] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (q < P.T && jc < P.S) am4[n] = *(const f32x4*)(arow + jc);
            }
        }
        bool k_all = true;                             // KM: every key of the tile is visible (wave-uniform)
        if constexpr (KM) {
            const uint32_t w = *(const uint32_t*)(smask + 4 * (lane & 15));
            if (__builtin_amdgcn_ballot_w64(w != 0u) == 0) continue;      // no visible key (the same in every wave)
            k_all = __builtin_amdgcn_ballot_w64(w != 0x01010101u) == 0;
        }

        f32x4 st[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < C::NKS; ++s) a = Tr<CT>::mma(read_rowfrag<CT>(kimg, C::STRIDE, 16 * n, s, lane), qf[s], a);
            st[n] = a;
            if constexpr (AM) st[n] += am4[n];
        }
        const int jb = kt * KT + 4 * g;                // key of element (n, r) is jb + 16n + r
        if (kt * KT + KT > lim_min) {                  // wave-uniform: only tiles that touch the mask edge pay for it
            const int rel = lim - jb;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) st[n][r] = (16 * n + r < rel) ? st[n][r] : -INFINITY;
        }
        if constexpr (KM) {
            if (!k_all) {
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const uint32_t w = *(const uint32_t*)(smask + 16 * n + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) st[n][r] = ((w >> (8 * r)) & 0xffu) ? st[n][r] : -INFINITY;
                }
            }
        }
        // 3-input maxima (v_max3_f32): two chains of four instead of a tree of fifteen 2-input ones
        auto max3 = [](float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); };
        float mx = max3(max3(max3(max3(st[0][0], st[0][1], st[0][2]), st[0][3], st[1][0]), st[1][1], st[1][2]), st[1][3], st[2][0]);
        float my = max3(max3(max3(st[2][1], st[2][2], st[2][3]), st[3][0], st[3][1]), st[3][2], st[3][3]);
        mx = fmaxf(mx, my);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float m_new = fmaxf(m_run, mx);
        // KM / AM: a query may have met no visible key yet (holes in front): keep the exponents finite, every p is exp2(-inf) = 0
        float m_use = m_new;
        if constexpr (KM || AM) m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = fast_exp2((m_run - m_use) * LOG2E);
        const float mneg = -m_use * LOG2E;
        m_run = m_new;
        // 4-wide float arithmetic compiles to packed-f32 VALU (v_pk_fma_f32 / v_pk_add_f32: two lanes of work per
        // instruction); only the exponentials stay scalar
        f32x4 ps4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const f32x4 e4 = st[n] * LOG2E + mneg;
            f32x4 p4;
#pragma unroll
            for (int r = 0; r < 4; ++r) p4[r] = fast_exp2(e4[r]);
            ps4 += p4;
            st[n] = p4;
        }
        const float psum = (ps4[0] + ps4[1]) + (ps4[2] + ps4[3]);
        // the probabilities leave each branch already packed as the PV operand (8 registers instead of 16 to merge: without
        // this the no-dropout path paid 16 v_mov per tile to meet the dropout path's register assignment)
        constexpr int NPF = KT / Tr<CT>::KSTEP;
        frag pf[NPF];
        if (dropping) {
            if (pair_ok) {                             // wave-uniform: r = 0..3 share one hash
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    float d0, d1, d2, d3;
                    bpm_drop_mult4(drop, drow + (uint32_t)(jb + 16 * n), d0, d1, d2, d3);
                    st[n] *= f32x4{d0, d1, d2, d3};
                }
            } else {
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int r = 0; r < 4; ++r) st[n][r] *= bpm_drop_mult(drop, drow + (uint32_t)(jb + 16 * n + r));
            }
#pragma unroll
            for (int ks = 0; ks < NPF; ++ks) pf[ks] = Tr<CT>::pack_rows(st, ks);
        } else {
#pragma unroll
            for (int ks = 0; ks < NPF; ++ks) pf[ks] = Tr<CT>::pack_rows(st, ks);
        }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int n = 0; n < C::ND; ++n) o[n] *= alpha;
        // O^T += V^T Pd^T : k = keys of this tile
        if (BPM_ATTN_SETPRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO + 1);
#pragma unroll
        for (int ks = 0; ks < NPF; ++ks) {
#pragma unroll
            for (int n = 0; n < C::ND; ++n)
                o[n] = Tr<CT>::mma(Tr<CT>::read_tr(vimg, C::STRIDE, ks * Tr<CT>::KSTEP, 16 * n, lane, Tr<CT>::TR_CTILE), pf[ks], o[n]);
        }
        if (BPM_ATTN_SETPRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    }
    l_run += __shfl_xor(l_run, 16);
    l_run += __shfl_xor(l_run, 32);
    // l_run >= 1 (the row maximum contributes exp(0)): v_log_f32 / v_rcp_f32 (1 ulp) without the library's denormal / division fix-ups
    if (q < P.T && g == 0) P.lse[(size_t)bh * P.T + q] = m_run + __builtin_amdgcn_logf(l_run) * 0.6931471805599453f;
    static_assert(2 * KT * C::STRIDE >= 4 * store_rows16_bytes<CT, DHP>(), "one transpose block per wave in the K / V images");
    __syncthreads();                                   // every wave is done with the K / V images
    if (q0 < P.T)
        store_rows16<CT, DHP>(smem + wave * store_rows16_bytes<CT, DHP>(), (CT*)P.O + ((size_t)q0 * P.B + b) * P.ldo + h * P.dh,
                              (size_t)P.B * P.ldo, P.T - q0, P.dh, o, __builtin_amdgcn_rcpf(l_run), lane);
}

// Two 64-row blocks per workgroup, b and nblk - 1 - b: under the future mask block b has b + 1 (forward / dQ) or nblk - b
// (dK / dV) tiles, so every pair carries the same work, and the per-block lead-in (operand loads, first tile, result
// store: ~6 us of latency that four resident workgroups per CU cannot hide) is paid half as often.  Measured on MI355X,
// 576 heads of 64, T = S = 512, masked: see DESIGN.md section 5 (attention).
template <typename CT, int DHP>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(attn_waves<CT>(0, DHP), attn_waves<CT>(0, DHP)))) void attn_fwd_kernel(const AGroup grp) {
    typedef Cfg<CT, DHP> C;
    __shared__ __attribute__((aligned(16))) char smem[2 * KT * C::STRIDE];
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const AProb& P = pick(grp, bid);
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const int nb2 = P.pair ? (P.nblk + 1) >> 1 : P.nblk;
    const int bh = bid / nb2, first = P.pair ? bid % nb2 : P.nblk - 1 - bid % nb2, second = P.pair ? P.nblk - 1 - first : first;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass && second == first) break;
        attn_fwd_block<CT, DHP, false>(P, drop, smem, bh, pass ? second : first, AMask{nullptr, 0});
    }
}

// the same schedule with a per-key mask (bpm_attn_fwd_kmask)
template <typename CT, int DHP>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(attn_waves<CT>(0, DHP), attn_waves<CT>(0, DHP)))) void attn_fwd_kmask_kernel(const AGroupK gk) {
    typedef Cfg<CT, DHP> C;
    __shared__ __attribute__((aligned(16))) char smem[2 * KT * C::STRIDE + KT];
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = pick_index(gk.g, bid);
    const AProb& P = gk.g.p[pi];
    const AMask km = gk.m[pi];
    const DropCfg drop = bpm_resolve_drop(P.drop, gk.g.seedp);
    const int nb2 = P.pair ? (P.nblk + 1) >> 1 : P.nblk;
    const int bh = bid / nb2, first = P.pair ? bid % nb2 : P.nblk - 1 - bid % nb2, second = P.pair ? P.nblk - 1 - first : first;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass && second == first) break;
        attn_fwd_block<CT, DHP, true>(P, drop, smem, bh, pass ? second : first, km);
    }
}

// ---------------------------------------------------------------------------
// backward, dQ (and delta = rowsum(dO * O))
// ---------------------------------------------------------------------------
// XP: also write dS and the dropped probabilities (AProb::dS / Pd) -- the few-query-row groups of the engine (level 2 under
// dead-row elimination) continue from those instead of dK / dV: with two query rows dK and dV have rank two per head, and
// every key / value-side product factors through [rows, S] matrices (engine.EncoderGroupPlan, "low-rank key side").
// A separate instantiation: the stores would cost the T = S = 512 launches registers.
// KM: per-key mask, staged as in the forward block (KTQ bytes of LDS behind the images).
// AM: additive mask, read as in the forward block (one float4 per 4 keys of the lane's query row) and added to the score
// before lse is subtracted: a -inf entry gives exp2(-inf) = 0 whatever lse is, so no guard is needed here.
template <typename CT, int DHP, bool XP, bool KM, bool AM = false>
BPM_DEV void attn_bwd_dq_block(const AProb& P, const DropCfg& drop, char* smem, const int bh, const int qb, const AMask km,
                               const AAdd am = AAdd{nullptr, 0, 0}) {
    typedef Cfg<CT, DHP> C;
    typedef typename Tr<CT>::frag frag;
    char* kimg = smem;
    char* vimg = smem + C::KTQ * C::STRIDE;
    uint8_t* smask = (uint8_t*)(smem + 2 * C::KTQ * C::STRIDE);    // KM only

    const int b = bh / P.H, h = bh % P.H;
    int tid_ = threadIdx.x;
    asm volatile("" : "+v"(tid_));                 // per-lane values are re-derived in each pass of the block-pair loop, not kept live across it
    const int tid = tid_, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int q0 = qb * 64 + wave * 16;
    const int q = q0 + c;
    const char* Qh = P.Q + (size_t)bh * P.T * C::ROWB;
    const char* dOh = P.dO + (size_t)bh * P.T * C::ROWB;
    const char* Kh = P.K + (size_t)bh * P.S * C::ROWB;
    const char* Vh = P.V + (size_t)bh * P.S * C::ROWB;

    frag qf[C::NKS], dof[C::NKS];
    float delta = 0.f;
    const bool o_wide = (P.dh % Tr<CT>::EPC) == 0 && (((uintptr_t)P.O | (uintptr_t)((size_t)P.ldo * C::SZ)) & 15) == 0;
#pragma unroll
    for (int s = 0; s < C::NKS; ++s) {
        qf[s] = load_frag<CT, DHP>(Qh, q, P.T, s, g);
        dof[s] = load_frag<CT, DHP>(dOh, q, P.T, s, g);
        if (q < P.T) {
            const CT* orow = (const CT*)P.O + ((size_t)q * P.B + b) * P.ldo + h * P.dh;
            const int d0 = s * Tr<CT>::KSTEP + g * Tr<CT>::EPC;
            if (o_wide) {                              // whole 16-byte chunks of the O row (element loads: one L2 request each)
                if (d0 < P.dh) {
                    const frag of = *(const frag*)(orow + d0);
#pragma unroll
                    for (int j = 0; j < Tr<CT>::EPC; ++j) delta += Tr<CT>::to_f(dof[s][j]) * Tr<CT>::to_f(of[j]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < Tr<CT>::EPC; ++j)
                    if (d0 + j < P.dh) delta += Tr<CT>::to_f(dof[s][j]) * Tr<CT>::to_f(orow[d0 + j]);
            }
        }
    }
    delta += __shfl_xor(delta, 16);
    delta += __shfl_xor(delta, 32);
    const float lse2 = (q < P.T) ? -P.lse[(size_t)bh * P.T + q] * LOG2E : 0.f;
    if (q < P.T && g == 0) P.delta[(size_t)bh * P.T + q] = delta;

    f32x4 dq[C::ND];
#pragma unroll
    for (int n = 0; n < C::ND; ++n) dq[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int q_hi = min(P.T, qb * 64 + 64) - 1;
    const int jend = min(P.S, P.qpos0 + q_hi * P.qstride + P.mask_off);
    const int ntile = (jend + C::KTQ - 1) / C::KTQ;
    const int lim = min(P.S, P.qpos0 + q * P.qstride + P.mask_off);
    const int lim_min = min(P.S, P.qpos0 + q0 * P.qstride + P.mask_off);
    const bool dropping = drop.thresh != 0;
    const uint32_t drow = ((uint32_t)bh * (uint32_t)P.T + (uint32_t)q) * (uint32_t)P.S;
    const bool pair_ok = (P.S & 3) == 0;               // row starts are multiples of 4: keys (4m .. 4m+3) are one hash quad

    RowStage<CT, DHP, C::KTQ> kst, vst;
    uint32_t n_vis = 0;                                // KM, threads < KTQ: next tile's visibility of key kt * KTQ + tid
    auto stage_mask = [&](int kt) {
        const int jm = kt * C::KTQ + tid;
        n_vis = 0;
        if (tid < C::KTQ && jm < P.S) n_vis = km.mask[(size_t)b * km.ldm + jm] != 0;
    };
    if (ntile > 0) {
        kst.load(Kh, 0, P.S, tid); vst.load(Vh, 0, P.S, tid);
        if constexpr (KM) stage_mask(0);
    }
    const float* arow = nullptr;                       // AM: this lane's mask row
    if constexpr (AM) arow = am.m + (size_t)h * am.hs + (size_t)min(q, P.T - 1) * am.ld;
#pragma unroll 1
    for (int kt = 0; kt < ntile; ++kt) {
        __syncthreads();
        kst.store(kimg, tid);
        vst.store(vimg, tid);
        if constexpr (KM) { if (tid < C::KTQ) smask[tid] = (uint8_t)n_vis; }
        __syncthreads();
        if (kt + 1 < ntile) {
            kst.load(Kh, (kt + 1) * C::KTQ, P.S, tid); vst.load(Vh, (kt + 1) * C::KTQ, P.S, tid);
            if constexpr (KM) stage_mask(kt + 1);
        }
        f32x4 am4[C::KTQ / 16];                        // AM: mask of keys kt * KTQ + 16n + 4g + (0..3)
        if constexpr (AM) {
#pragma unroll
            for (int n = 0; n < C::KTQ / 16; ++n) {
                const int jc = kt * C::KTQ + 16 * n + 4 * g;    // jc % 4 == 0 and ldm % 4 == 0: jc < S implies jc + 3 < ldm
                am4[n] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (q < P.T && jc < P.S) am4[n] = *(const f32x4*)(arow + jc);
            }
        }
        bool k_all = true;                             // KM: every key of the tile is visible (wave-uniform)
        if constexpr (KM) {
            const uint32_t w = *(const uint32_t*)(smask + 4 * (lane & (C::KTQ / 4 - 1)));
            if (__builtin_amdgcn_ballot_w64(w != 0u) == 0) continue;      // no visible key (the same in every wave)
            k_all = __builtin_amdgcn_ballot_w64(w != 0x01010101u) == 0;
        }
        const int jb = kt * C::KTQ + 4 * g;
        const bool edge = kt * C::KTQ + C::KTQ > lim_min;
        const int rel = lim - jb;
        // one k-step of the dQ product (32 keys in bf16, 16 in f32) at a time: its dS lives only until its MFMAs
        constexpr int NPK = Tr<CT>::KSTEP / 16;
#pragma unroll
        for (int ks = 0; ks < C::KTQ / Tr<CT>::KSTEP; ++ks) {
            f32x4 ds[NPK];
#pragma unroll
            for (int nn = 0; nn < NPK; ++nn) {
                const int n = ks * NPK + nn;
                f32x4 s_ = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < C::NKS; ++s) {
                    s_ = Tr<CT>::mma(read_rowfrag<CT>(kimg, C::STRIDE, 16 * n, s, lane), qf[s], s_);
                    dp = Tr<CT>::mma(read_rowfrag<CT>(vimg, C::STRIDE, 16 * n, s, lane), dof[s], dp);
                }
                if constexpr (AM) s_ += am4[n];
                float dm[4] = {1.f, 1.f, 1.f, 1.f};
                if (dropping) {
                    if (pair_ok) {
                        bpm_drop_mult4(drop, drow + (uint32_t)(jb + 16 * n), dm[0], dm[1], dm[2], dm[3]);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) dm[r] = bpm_drop_mult(drop, drow + (uint32_t)(jb + 16 * n + r));
                    }
                }
                f32x4 e4 = s_ * LOG2E + lse2;
                if (edge) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) e4[r] = (16 * n + r < rel) ? e4[r] : -INFINITY;   // exp2(-inf) = 0: masked before the exponential
                }
                if constexpr (KM) {
                    if (!k_all) {
                        const uint32_t w = *(const uint32_t*)(smask + 16 * n + 4 * g);
#pragma unroll
                        for (int r = 0; r < 4; ++r) e4[r] = ((w >> (8 * r)) & 0xffu) ? e4[r] : -INFINITY;
                    }
                }
                f32x4 p4;
#pragma unroll
                for (int r = 0; r < 4; ++r) p4[r] = fast_exp2(e4[r]);
                const f32x4 dm4 = f32x4{dm[0], dm[1], dm[2], dm[3]};
                ds[nn] = p4 * (dp * dm4 - delta);
                if constexpr (XP) {
                    const int j0 = jb + 16 * n;                  // four consecutive keys (S % 4 == 0: all four or none exist)
                    if (P.dS && q < P.T && j0 < P.S) {
                        const size_t off = (size_t)b * P.xs_b + (size_t)h * P.xs_h + (size_t)q * P.xs_q + j0;
                        const f32x4 pd = p4 * dm4;
                        if constexpr (C::SZ == 4) {
                            *(f32x4*)((float*)P.dS + off) = ds[nn];
                            *(f32x4*)((float*)P.Pd + off) = pd;
                        } else {
                            bf16x4 o, w;
#pragma unroll
                            for (int r = 0; r < 4; ++r) { o[r] = (bf16_t)ds[nn][r]; w[r] = (bf16_t)pd[r]; }
                            *(bf16x4*)((bf16_t*)P.dS + off) = o;
                            *(bf16x4*)((bf16_t*)P.Pd + off) = w;
                        }
                    }
                }
            }
            // dQ^T += K^T dS^T
            if (BPM_ATTN_SETPRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO + 1);
            const frag df = Tr<CT>::pack_rows(ds, 0);
#pragma unroll
            for (int n = 0; n < C::ND; ++n)
                dq[n] = Tr<CT>::mma(Tr<CT>::read_tr(kimg, C::STRIDE, ks * Tr<CT>::KSTEP, 16 * n, lane, Tr<CT>::TR_CTILE), df, dq[n]);
            if (BPM_ATTN_SETPRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
        }
    }
    static_assert(2 * C::KTQ * C::STRIDE >= 4 * store_rows16_bytes<CT, DHP>(), "one transpose block per wave in the K / V images");
    __syncthreads();                                   // every wave is done with the K / V images
    if (q0 < P.T)
        store_rows16<CT, DHP>(smem + wave * store_rows16_bytes<CT, DHP>(), (CT*)P.dQ + ((size_t)q0 * P.B + b) * P.lddq + h * P.dh,
                              (size_t)P.B * P.lddq, P.T - q0, P.dh, dq, P.dq_scale, lane);
}

// Two 64-row blocks per workgroup, b and nblk - 1 - b: under the future mask block b has b + 1 (forward / dQ) or nblk - b
// (dK / dV) tiles, so every pair carries the same work, and the per-block lead-in (operand loads, first tile, result
// store: ~6 us of latency that four resident workgroups per CU cannot hide) is paid half as often.  Measured on MI355X,
// 576 heads of 64, T = S = 512, masked: see DESIGN.md section 5 (attention).
template <typename CT, int DHP, bool XP>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(attn_waves<CT>(1, DHP), attn_waves<CT>(1, DHP)))) void attn_bwd_dq_kernel(const AGroup grp) {
    typedef Cfg<CT, DHP> C;
    __shared__ __attribute__((aligned(16))) char smem[2 * C::KTQ * C::STRIDE];
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const AProb& P = pick(grp, bid);
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const int nb2 = P.pair ? (P.nblk + 1) >> 1 : P.nblk;
    const int bh = bid / nb2, first = P.pair ? bid % nb2 : P.nblk - 1 - bid % nb2, second = P.pair ? P.nblk - 1 - first : first;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass && second == first) break;
        attn_bwd_dq_block<CT, DHP, XP, false>(P, drop, smem, bh, pass ? second : first, AMask{nullptr, 0});
    }
}

// the same schedule with a per-key mask (bpm_attn_bwd_dq_kmask)
template <typename CT, int DHP>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(attn_waves<CT>(1, DHP), attn_waves<CT>(1, DHP)))) void attn_bwd_dq_kmask_kernel(const AGroupK gk) {
    typedef Cfg<CT, DHP> C;
    __shared__ __attribute__((aligned(16))) char smem[2 * C::KTQ * C::STRIDE + C::KTQ];
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = pick_index(gk.g, bid);
    const AProb& P = gk.g.p[pi];
    const AMask km = gk.m[pi];
    const DropCfg drop = bpm_resolve_drop(P.drop, gk.g.seedp);
    const int nb2 = P.pair ? (P.nblk + 1) >> 1 : P.nblk;
    const int bh = bid / nb2, first = P.pair ? bid % nb2 : P.nblk - 1 - bid % nb2, second = P.pair ? P.nblk - 1 - first : first;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass && second == first) break;
        attn_bwd_dq_block<CT, DHP, false, true>(P, drop, smem, bh, pass ? second : first, km);
    }
}

// ---------------------------------------------------------------------------
// backward, dK and dV
// ---------------------------------------------------------------------------
// KM: per-key mask.  A lane owns one key: its byte is read once (never at j >= S); a hidden key sees no query row
// (ilo past every row), so its probabilities are exp2(-inf) = 0 and its dK / dV rows are exact zeros.  A block without
// any visible key skips its query tiles.
// AM: additive mask through its transpose (AAdd holds maskT [S, ldt]): the lane's key row, one float4 per 4 queries of a
// register group, never read at j >= S or at a group that starts at i >= T.  A -inf entry gives probability 0, so the
// pair adds exactly nothing to dK / dV.
template <typename CT, int DHP, bool KM, bool AM = false>
BPM_DEV void attn_bwd_dkv_block(const AProb& P, const DropCfg& drop, char* smem, const int bh, const int kb, const AMask km,
                                const AAdd am = AAdd{nullptr, 0, 0}) {
    typedef Cfg<CT, DHP> C;
    typedef typename Tr<CT>::frag frag;
    char* qimg = smem;
    char* doimg = smem + C::QTK * C::STRIDE;
    float* s_lse = (float*)(smem + 2 * C::QTK * C::STRIDE);      // -lse * log2(e)
    float* s_del = s_lse + C::QTK;

    const int b = bh / P.H, h = bh % P.H;
    int tid_ = threadIdx.x;
    asm volatile("" : "+v"(tid_));                 // per-lane values are re-derived in each pass of the block-pair loop, not kept live across it
    const int tid = tid_, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int j0 = kb * 64 + wave * 16;                // wave-uniform first key
    const int j = j0 + c;                              // this lane's key
    const char* Qh = P.Q + (size_t)bh * P.T * C::ROWB;
    const char* dOh = P.dO + (size_t)bh * P.T * C::ROWB;
    const char* Kh = P.K + (size_t)bh * P.S * C::ROWB;
    const char* Vh = P.V + (size_t)bh * P.S * C::ROWB;

    frag kf[C::NKS], vf[C::NKS];
#pragma unroll
    for (int s = 0; s < C::NKS; ++s) {
        kf[s] = load_frag<CT, DHP>(Kh, j, P.S, s, g);
        vf[s] = load_frag<CT, DHP>(Vh, j, P.S, s, g);
    }
    f32x4 dk[C::ND], dv[C::ND];
#pragma unroll
    for (int n = 0; n < C::ND; ++n) { dk[n] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[n] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    // query i sees key j iff i >= ilo = j - mask_off + 1 (and i < T, j < S)
    // in ROW indices: row i sits at time qpos0 + i*qstride, so "time >= tmin" is "i >= ceil((tmin - qpos0) / qstride)"
    auto first_row = [&](int tmin) { const int a = tmin - P.qpos0; return a <= 0 ? 0 : (a + P.qstride - 1) / P.qstride; };
    int ilo = (j < P.S) ? first_row(j - P.mask_off + 1) : (1 << 30);
    int ilo_max = (j0 + 15 < P.S) ? first_row(j0 + 15 - P.mask_off + 1) : (1 << 30);         // wave-uniform: tiles at or above it need no test
    const int i_first = first_row(kb * 64 - P.mask_off + 1);                                   // first query row that sees any key of the block
    const int qt_lo = i_first / C::QTK;
    int qt_hi = (P.T + C::QTK - 1) / C::QTK;
    if constexpr (KM) {
        bool kvis = false;
        if (j < P.S) kvis = km.mask[(size_t)b * km.ldm + j] != 0;
        if (!kvis) ilo = 1 << 30;
        if (__builtin_amdgcn_ballot_w64(!kvis) != 0) ilo_max = 1 << 30;                        // a hidden key in the wave: every tile tests
        if (!__syncthreads_or(kvis)) qt_hi = qt_lo;                                            // block-uniform: nothing to do but store zeros
    }
    const bool dropping = drop.thresh != 0;
    const bool pair_ok = (P.S & 3) == 0;               // row starts are multiples of 4: keys (4m .. 4m+3) are one hash quad

    RowStage<CT, DHP, C::QTK> qst, dost;
    float n_lse = 0.f, n_del = 0.f;                    // threads < QTK: next tile's -lse*log2(e) and delta
    const float* lse_h = P.lse + (size_t)bh * P.T;
    const float* del_h = P.delta + (size_t)bh * P.T;
    auto stage = [&](int qt) {
        qst.load(Qh, qt * C::QTK, P.T, tid);
        dost.load(dOh, qt * C::QTK, P.T, tid);
        const int i = qt * C::QTK + (tid & (C::QTK - 1));
        const bool ok = i < P.T;
        const float l = lse_h[ok ? i : 0], dl = del_h[ok ? i : 0];
        n_lse = ok ? -l * LOG2E : 0.f;
        n_del = ok ? dl : 0.f;
    };
    if (qt_lo < qt_hi) stage(qt_lo);
    const float* acol = nullptr;                       // AM: this lane's row of the transposed mask
    if constexpr (AM) acol = am.m + (size_t)h * am.hs + (size_t)min(j, P.S - 1) * am.ld;
#pragma unroll 1
    for (int qt = qt_lo; qt < qt_hi; ++qt) {
        __syncthreads();
        qst.store(qimg, tid);
        dost.store(doimg, tid);
        if (tid < C::QTK) { s_lse[tid] = n_lse; s_del[tid] = n_del; }
        __syncthreads();
        if (qt + 1 < qt_hi) stage(qt + 1);
        f32x4 am4[C::QTK / 16];                        // AM: mask of queries qt * QTK + 16u + 4g + (0..3) against key j
        if constexpr (AM) {
#pragma unroll
            for (int u = 0; u < C::QTK / 16; ++u) {
                const int ic = qt * C::QTK + 16 * u + 4 * g;    // ic % 4 == 0 and ldt % 4 == 0: ic < T implies ic + 3 < ldt
                am4[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (j < P.S && ic < P.T) am4[u] = *(const f32x4*)(acol + ic);
            }
        }
        const bool edge = (qt * C::QTK < ilo_max) || (qt * C::QTK + C::QTK > P.T);
        // one k-step of the dV / dK products (32 queries in bf16, 16 in f32) at a time: its scores, probabilities and
        // dS live only until its MFMAs (half the registers of doing the whole 64-query tile first)
        constexpr int UPK = Tr<CT>::KSTEP / 16;
#pragma unroll
        for (int ks = 0; ks < C::QTK / Tr<CT>::KSTEP; ++ks) {
            f32x4 pd[UPK], ds[UPK];
#pragma unroll
            for (int uu = 0; uu < UPK; ++uu) {
                const int u = ks * UPK + uu;
                f32x4 s_ = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < C::NKS; ++s) {
                    s_ = Tr<CT>::mma(read_rowfrag<CT>(qimg, C::STRIDE, 16 * u, s, lane), kf[s], s_);
                    dp = Tr<CT>::mma(read_rowfrag<CT>(doimg, C::STRIDE, 16 * u, s, lane), vf[s], dp);
                }
                if constexpr (AM) s_ += am4[u];
                const f32x4 l4 = *(const f32x4*)(s_lse + 16 * u + 4 * g);
                const f32x4 d4 = *(const f32x4*)(s_del + 16 * u + 4 * g);
                const int ib = qt * C::QTK + 16 * u + 4 * g;       // query of element r is ib + r
                f32x4 e4 = s_ * LOG2E + l4;
                if (edge) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) e4[r] = (ib + r >= ilo && ib + r < P.T) ? e4[r] : -INFINITY;
                }
                f32x4 p4, dm4 = f32x4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
                for (int r = 0; r < 4; ++r) p4[r] = fast_exp2(e4[r]);
                if (dropping) {
                    if (pair_ok) {
                        // Element (query ib + r, key j) is 16-bit lane j & 3 of the hash quad (query, j >> 2) -- the quads the
                        // forward / dQ kernels draw once per four KEYS.  Here a lane holds four QUERIES of one key: four quads.
                        // The four lanes of a DPP quad hold keys 4m .. 4m + 3, so they need the same four quads: lane c hashes
                        // the one of query ib + (c & 3) and the others come over DPP (quad_perm broadcast): one hash
                        // (3 quarter-rate multiplies) per lane and step instead of four.
                        uint32_t w0, w1;
                        bpm_hash64((((uint32_t)bh * (uint32_t)P.T + (uint32_t)(ib + (c & 3))) * (uint32_t)P.S + (uint32_t)j) >> 2, drop.key, w0, w1);
                        const bool hi_word = (j & 2) != 0, hi_half = (j & 1) != 0;
                        auto from = [&](auto R) {
                            constexpr int r = decltype(R)::value;
                            const uint32_t a0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w0, 0x55 * r, 0xf, 0xf, false);
                            const uint32_t a1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w1, 0x55 * r, 0xf, 0xf, false);
                            const uint32_t w = hi_word ? a1 : a0;
                            const uint32_t bits = hi_half ? (w >> 16) : (w & 0xFFFFu);
                            dm4[r] = bits < drop.thresh ? 0.0f : drop.inv_keep;
                        };
                        from(std::integral_constant<int, 0>{}); from(std::integral_constant<int, 1>{});
                        from(std::integral_constant<int, 2>{}); from(std::integral_constant<int, 3>{});
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            dm4[r] = bpm_drop_mult(drop, ((uint32_t)bh * (uint32_t)P.T + (uint32_t)(ib + r)) * (uint32_t)P.S + (uint32_t)j);
                    }
                }
                pd[uu] = p4 * dm4;
                ds[uu] = p4 * (dp * dm4 - d4);
            }
            if (BPM_ATTN_SETPRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO + 1);
            const frag pf = Tr<CT>::pack_rows(pd, 0);
            const frag df = Tr<CT>::pack_rows(ds, 0);
#pragma unroll
            for (int n = 0; n < C::ND; ++n) {
                dv[n] = Tr<CT>::mma(Tr<CT>::read_tr(doimg, C::STRIDE, ks * Tr<CT>::KSTEP, 16 * n, lane, Tr<CT>::TR_CTILE), pf, dv[n]);
                dk[n] = Tr<CT>::mma(Tr<CT>::read_tr(qimg, C::STRIDE, ks * Tr<CT>::KSTEP, 16 * n, lane, Tr<CT>::TR_CTILE), df, dk[n]);
            }
            if (BPM_ATTN_SETPRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
        }
    }
    static_assert(2 * C::QTK * C::STRIDE >= 4 * store_rows16_bytes<CT, DHP>(), "one transpose block per wave in the Q / dO images");
    __syncthreads();                                   // every wave is done with the Q / dO images
    if (j0 < P.S) {
        char* blk = smem + wave * store_rows16_bytes<CT, DHP>();
        store_rows16<CT, DHP>(blk, (CT*)P.dK + ((size_t)j0 * P.B + b) * P.lddk + h * P.dh, (size_t)P.B * P.lddk, P.S - j0, P.dh, dk, 1.f, lane);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the block is read out before dV overwrites it
        store_rows16<CT, DHP>(blk, (CT*)P.dV + ((size_t)j0 * P.B + b) * P.lddv + h * P.dh, (size_t)P.B * P.lddv, P.S - j0, P.dh, dv, 1.f, lane);
    }
}

// Two 64-row blocks per workgroup, b and nblk - 1 - b: under the future mask block b has b + 1 (forward / dQ) or nblk - b
// (dK / dV) tiles, so every pair carries the same work, and the per-block lead-in (operand loads, first tile, result
// store: ~6 us of latency that four resident workgroups per CU cannot hide) is paid half as often.  Measured on MI355X,
// 576 heads of 64, T = S = 512, masked: see DESIGN.md section 5 (attention).
template <typename CT, int DHP>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(attn_waves<CT>(2, DHP), attn_waves<CT>(2, DHP)))) void attn_bwd_dkv_kernel(const AGroup grp) {
    typedef Cfg<CT, DHP> C;
    __shared__ __attribute__((aligned(16))) char smem[2 * C::QTK * C::STRIDE + 2 * C::QTK * 4];
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const AProb& P = pick(grp, bid);
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const int nb2 = P.pair ? (P.nblk + 1) >> 1 : P.nblk;
    const int bh = bid / nb2, first = P.pair ? bid % nb2 : bid % nb2, second = P.pair ? P.nblk - 1 - first : first;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass && second == first) break;
        attn_bwd_dkv_block<CT, DHP, false>(P, drop, smem, bh, pass ? second : first, AMask{nullptr, 0});
    }
}

// the same schedule with a per-key mask (bpm_attn_bwd_dkv_kmask)
template <typename CT, int DHP>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(attn_waves<CT>(2, DHP), attn_waves<CT>(2, DHP)))) void attn_bwd_dkv_kmask_kernel(const AGroupK gk) {
    typedef Cfg<CT, DHP> C;
    __shared__ __attribute__((aligned(16))) char smem[2 * C::QTK * C::STRIDE + 2 * C::QTK * 4];
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = pick_index(gk.g, bid);
    const AProb& P = gk.g.p[pi];
    const AMask km = gk.m[pi];
    const DropCfg drop = bpm_resolve_drop(P.drop, gk.g.seedp);
    const int nb2 = P.pair ? (P.nblk + 1) >> 1 : P.nblk;
    const int bh = bid / nb2, first = P.pair ? bid % nb2 : bid % nb2, second = P.pair ? P.nblk - 1 - first : first;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass && second == first) break;
        attn_bwd_dkv_block<CT, DHP, true>(P, drop, smem, bh, pass ? second : first, km);
    }
}

// ---------------------------------------------------------------------------
// the three kernels with an additive mask (bpm_attn_fwd_amask / _bwd_dq_amask / _bwd_dkv_amask)
// ---------------------------------------------------------------------------
// The same schedules, compiled for the occupancy of their unmasked siblings: the tile's mask values are 16 more live
// registers (8 in the 32-row tiles of head_dim 256), which the allocator finds in 21 of the 24 instantiations without
// scratch.  bf16 dK / dV at head_dim 64 spills 20 bytes per lane at three waves and bf16 dQ at 128 spills 32 at three:
// measured at the first (MI355X, T = S = 512, all-zeros mask) 134 us at three waves against 146 - 151 at two without
// spills, so both stay.  f32 dK / dV at head_dim 128 would spill 228 bytes at two waves: that one is compiled for one.
template <typename CT>
constexpr int attn_waves_am(int kernel, int dhp) {
    return (sizeof(CT) == 4 && kernel == 2 && dhp == 128) ? 1 : attn_waves<CT>(kernel, dhp);
}

template <typename CT, int DHP, int WHICH>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(attn_waves_am<CT>(WHICH, DHP), attn_waves_am<CT>(WHICH, DHP)))) void attn_amask_kernel(const AGroupA ga) {
    typedef Cfg<CT, DHP> C;
    constexpr int ROWS = WHICH == 0 ? KT : WHICH == 1 ? C::KTQ : C::QTK;
    __shared__ __attribute__((aligned(16))) char smem[2 * ROWS * C::STRIDE + (WHICH == 2 ? 2 * C::QTK * 4 : 0)];
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = pick_index(ga.g, bid);
    const AProb& P = ga.g.p[pi];
    const AAdd am = ga.m[pi];
    const DropCfg drop = bpm_resolve_drop(P.drop, ga.g.seedp);
    const int nb2 = P.pair ? (P.nblk + 1) >> 1 : P.nblk;
    const int bh = bid / nb2;
    const int first = (P.pair || WHICH == 2) ? bid % nb2 : P.nblk - 1 - bid % nb2, second = P.pair ? P.nblk - 1 - first : first;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass && second == first) break;
        const int blk = pass ? second : first;
        if constexpr (WHICH == 0) attn_fwd_block<CT, DHP, false, true>(P, drop, smem, bh, blk, AMask{nullptr, 0}, am);
        else if constexpr (WHICH == 1) attn_bwd_dq_block<CT, DHP, false, false, true>(P, drop, smem, bh, blk, AMask{nullptr, 0}, am);
        else attn_bwd_dkv_block<CT, DHP, false, true>(P, drop, smem, bh, blk, AMask{nullptr, 0}, am);
    }
}

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
static_assert(sizeof(MGroupA) <= 4096, "kernel arguments are limited to 4 KiB");
BPM_DEV const MGroup& map_group(const MGroup& g) { return g; }
BPM_DEV const MGroup& map_group(const MGroupA& g) { return g.g; }

template <typename CT, int DHP, bool AM = false, bool PH = false>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(map_waves<CT>(DHP, AM), map_waves<CT>(DHP, AM)))) void attn_maps_kernel(const std::conditional_t<AM, MGroupA, MGroup> ga) {
    static_assert(AM || !PH, "a head stride belongs to an additive mask");
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
    const int ilo = (j < P.S) ? first_row(j - P.mask_off + 1) : (1 << 30);
    const int ilo_max = (j0 + 15 < P.S) ? first_row(j0 + 15 - P.mask_off + 1) : (1 << 30);   // wave-uniform: rows at or above it need no test
    const int i_first = first_row(kb * 64 - P.mask_off + 1);                                   // first query row that sees any key of the tile
    const int i_end = min(P.T, i0 + MQT);

    f32x4 acc[MQT / 16];
#pragma unroll
    for (int u = 0; u < MQT / 16; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (i_first < i_end) {                              // block-uniform: a fully masked tile keeps its zeros
        f32x4 am4[MQT / 16];                            // AM: mask of queries i0 + 16u + 4g + (0..3) against key j
        AAdd am = AAdd{nullptr, 0, 0};
        if constexpr (AM) am = ga.m[pi];
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

template <typename CT, int DHP>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(dbias_waves<CT>(DHP), dbias_waves<CT>(DHP)))) void attn_dbias_kernel(const DGroup grp) {
    typedef Cfg<CT, DHP> C;
    typedef typename Tr<CT>::frag frag;
    __shared__ __attribute__((aligned(16))) char smem[2 * KT * C::STRIDE];
    char* kimg = smem;
    char* vimg = smem + KT * C::STRIDE;

    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int pi = 0;
#pragma unroll 1
    for (int i = 1; i < grp.nprob; ++i)
        if (bid >= grp.p[i].blk0) pi = i;
    const DProb& P = grp.p[pi];
    bid -= P.blk0;
    const DropCfg drop = bpm_resolve_drop(P.drop, grp.seedp);
    const int kt = bid % P.nkt, qb = (bid / P.nkt) % P.nqt;                 // key tiles of a query tile are neighbours
    const int rest = bid / (P.nkt * P.nqt), sp = rest % P.nsplit, img = rest / P.nsplit;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int q0 = qb * 64 + wave * 16;               // wave-uniform first query
    const int q = q0 + c;                             // this lane's query
    const int jb = kt * KT + 4 * g;                   // key of element (n, r) is jb + 16n + r

    f32x4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int q_hi = min(P.T, qb * 64 + 64) - 1;
    const int jend = min(P.S, P.qpos0 + q_hi * P.qstride + P.mask_off);      // one past the last key any query of this tile sees
    const int lim = min(P.S, P.qpos0 + q * P.qstride + P.mask_off);          // this lane sees keys j < lim
    const int lim_min = min(P.S, P.qpos0 + q0 * P.qstride + P.mask_off);     // every lane of the wave sees keys j < lim_min
    const bool edge = kt * KT + KT > lim_min;
    const int rel = lim - jb;
    const bool dropping = drop.thresh != 0;
    const bool pair_ok = (P.S & 3) == 0;               // row starts are multiples of 4: keys (4m .. 4m+3) are one hash quad
    const int t0 = sp * P.chunk, t1 = min(P.nterm, t0 + P.chunk);
    auto head_of = [&](int t) { return P.per_head ? t * P.H + img : t; };    // term -> (b * H + h)

    if (kt * KT < jend && t0 < t1) {                   // block-uniform: a tile the mask_off rule hides keeps its zeros
        RowStage<CT, DHP, KT> kst, vst;
        auto stage = [&](int t) {
            const size_t bh = (size_t)head_of(t);
            kst.load(P.K + bh * P.S * C::ROWB, kt * KT, P.S, tid);
            vst.load(P.V + bh * P.S * C::ROWB, kt * KT, P.S, tid);
        };
        stage(t0);
#pragma unroll 1
        for (int t = t0; t < t1; ++t) {
            const int bh = head_of(t), h = bh % P.H;
            // this head's operands of the lane's query: issued before the barriers, used after them
            frag qf[C::NKS], dof[C::NKS];
            const char* Qh = P.Q + (size_t)bh * P.T * C::ROWB;
            const char* dOh = P.dO + (size_t)bh * P.T * C::ROWB;
#pragma unroll
            for (int s = 0; s < C::NKS; ++s) {
                qf[s] = load_frag<CT, DHP>(Qh, q, P.T, s, g);
                dof[s] = load_frag<CT, DHP>(dOh, q, P.T, s, g);
            }
            const size_t srow = (size_t)bh * P.T + min(q, P.T - 1);
            const float lse2 = (q < P.T) ? -P.lse[srow] * LOG2E : 0.f;
            const float delta = (q < P.T) ? P.delta[srow] : 0.f;
            const float* arow = P.m + (size_t)h * P.mhs + (size_t)min(q, P.T - 1) * P.ldm;
            f32x4 am4[4];                              // mask of keys kt * KT + 16n + 4g + (0..3)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int jc = jb + 16 * n;            // jc % 4 == 0 and ldm % 4 == 0: jc < S implies jc + 3 < ldm
                am4[n] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (q < P.T && jc < P.S) am4[n] = *(const f32x4*)(arow + jc);
            }
            __syncthreads();                           // every wave is done with the previous head's images
            kst.store(kimg, tid);
            vst.store(vimg, tid);
            __syncthreads();
            if (t + 1 < t1) stage(t + 1);
            const uint32_t drow = ((uint32_t)bh * (uint32_t)P.T + (uint32_t)q) * (uint32_t)P.S;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                f32x4 s_ = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < C::NKS; ++s) {
                    s_ = Tr<CT>::mma(read_rowfrag<CT>(kimg, C::STRIDE, 16 * n, s, lane), qf[s], s_);
                    dp = Tr<CT>::mma(read_rowfrag<CT>(vimg, C::STRIDE, 16 * n, s, lane), dof[s], dp);
                }
                s_ += am4[n];
                float dm[4] = {1.f, 1.f, 1.f, 1.f};
                if (dropping) {
                    if (pair_ok) {
                        bpm_drop_mult4(drop, drow + (uint32_t)(jb + 16 * n), dm[0], dm[1], dm[2], dm[3]);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) dm[r] = bpm_drop_mult(drop, drow + (uint32_t)(jb + 16 * n + r));
                    }
                }
                f32x4 e4 = s_ * LOG2E + lse2;
                if (edge) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) e4[r] = (16 * n + r < rel) ? e4[r] : -INFINITY;   // exp2(-inf) = 0: masked before the exponential
                }
                f32x4 p4;
#pragma unroll
                for (int r = 0; r < 4; ++r) p4[r] = fast_exp2(e4[r]);
                const f32x4 dm4 = f32x4{dm[0], dm[1], dm[2], dm[3]};
                acc[n] += p4 * (dp * dm4 - delta);
            }
        }
    }
    if (q < P.T) {
        float* orow = P.out + (size_t)sp * P.osplit + (size_t)img * P.ohs + (size_t)q * P.ldo;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int jc = jb + 16 * n;
            if (jc + 4 <= P.wlim) *(f32x4*)(orow + jc) = acc[n];
            else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (jc + r < P.wlim) orow[jc + r] = acc[n][r];
            }
        }
    }
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

__global__ __launch_bounds__(NTHREADS) void attn_dbias_sum_kernel(const DSumGroup grp) {
    unsigned bid = blockIdx.x;
    int pi = 0;
#pragma unroll 1
    for (int i = 1; i < grp.nprob; ++i)
        if (bid >= grp.p[i].blk0) pi = i;
    const DSumProb& P = grp.p[pi];
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
    float* dst = P.dB + (size_t)img * P.ohs + (size_t)i * P.lddb + j;
    if (j + 4 <= P.S) *(f32x4*)dst = v;
    else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (j + r < P.S) dst[r] = v[r];
    }
}

// tuning hook (tools/attn_lab.py): bit k = kernel k (0 forward, 1 dQ, 2 dK/dV) pairs blocks
// bit k: kernel k (forward, dQ, dK/dV) takes two 64-row blocks per workgroup.  A constant in the product library; a
// -DBPM_LAB build (tools/attn_lab.py, the block-pairing test) can switch it through bpm_debug_attn_pair.
#ifdef BPM_LAB
int g_attn_pair = 7;
#else
constexpr int g_attn_pair = 7;
#endif

int fill(AGroup& g, const bpm_attn_problem* probs, int nprob, int blocks_over_S, uint64_t seed, int* total, int kernel) {
    if (nprob < 1 || nprob > BPM_MAX_GROUP || !probs) return BPM_ERR_ARG;
    g.nprob = nprob;
    g.seedp = bpm_seed_ptr(seed);
    int blk = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        AProb& p = g.p[i];
        if (q.B < 1 || q.H < 1 || q.T < 1 || q.S < 1 || q.dh < 1 || q.dh > q.dhp) return BPM_ERR_ARG;
        if (q.T > (1 << 22) || q.S > (1 << 22)) return BPM_ERR_ARG;      // index arithmetic is 32-bit (rows * 512 B per head fits 31 bits)
        if ((long)(q.T > q.S ? q.T : q.S) * q.dhp * 4 > (1l << 31)) return BPM_ERR_ARG;   // ... and rows * 1 KiB at head_dim 256 in f32
        if (q.dhp != probs[0].dhp) return BPM_ERR_ARG;
        p.Q = (const char*)q.Q; p.K = (const char*)q.K; p.V = (const char*)q.V;
        p.O = (char*)q.O; p.ldo = q.ldo; p.lse = q.lse;
        p.dO = (const char*)q.dO; p.delta = q.delta;
        p.dQ = (char*)q.dQ; p.lddq = q.lddq; p.dK = (char*)q.dK; p.lddk = q.lddk; p.dV = (char*)q.dV; p.lddv = q.lddv;
        p.B = q.B; p.H = q.H; p.T = q.T; p.S = q.S; p.dh = q.dh;
        p.mask_off = (q.mask_off > 0 && q.mask_off < (1 << 29)) ? q.mask_off : (1 << 29);
        if (q.q_pos0 < 0 || q.q_stride < 0 || q.q_pos0 > (1 << 24) || q.q_stride > (1 << 24)) return BPM_ERR_ARG;
        p.qpos0 = q.q_pos0; p.qstride = q.q_stride > 0 ? q.q_stride : 1;
        if ((long)p.qpos0 + (long)(q.T - 1) * p.qstride > (1l << 28)) return BPM_ERR_ARG;
        p.dq_scale = q.dq_scale;
        p.dS = (char*)q.dS; p.Pd = (char*)q.Pd; p.xs_b = q.xs_b; p.xs_h = q.xs_h; p.xs_q = q.xs_q;
        if (q.dS || q.Pd) {       // both, whole 4-key groups, 4-element-aligned rows that do not run into each other
            if (!q.dS || !q.Pd || (q.S & 3) || ((q.xs_b | q.xs_h | q.xs_q) & 3) || q.xs_b < 0 || q.xs_h < 0 || q.xs_q < q.S) return BPM_ERR_ARG;
            if ((((uintptr_t)q.dS | (uintptr_t)q.Pd) & 15) != 0) return BPM_ERR_ALIGN;
        }
        p.drop = bpm_make_drop(q.drop_p, seed, q.drop_site);
        p.nblk = ((blocks_over_S ? q.S : q.T) + 63) / 64;
        p.blk0 = blk;
        p.pair = (g_attn_pair >> kernel) & 1;
        blk += (p.pair ? (p.nblk + 1) >> 1 : p.nblk) * q.B * q.H;
    }
    *total = blk;
    return 0;
}

// sum over problems of B*H*dh * (number of visible (query, key) pairs): the useful
// multiply-adds of ONE attention product (P(T,S) = sum_i min(S, i + mask_off))
double useful_pair_flops(const bpm_attn_problem* probs, int nprob) {
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

// algorithmic HBM bytes of one launch: every tensor it must read or write once (which: 0 forward, 1 dQ + delta, 2 dK / dV)
double attn_bytes(const bpm_attn_problem* probs, int nprob, int sz, int which) {
    double tot = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        const double bh = (double)q.B * q.H, qe = bh * q.T * q.dh * sz, ke = bh * q.S * q.dh * sz, st = bh * q.T * 4;
        if (which == 0) tot += 2 * qe + 2 * ke + st;                 // Q, K, V in; O, lse out
        else if (which == 1) tot += 4 * qe + 2 * ke + 2 * st;        // Q, K, V, O, dO, lse in; dQ, delta out
        else tot += 2 * qe + 4 * ke + 2 * st;                        // Q, K, V, dO, lse, delta in; dK, dV out
    }
    return tot;
}

template <typename CT>
int dispatch(int which, int dhp, const AGroup& g, int total, hipStream_t s) {
    dim3 grid(total), block(NTHREADS);
#define BPM_ATTN_CASE(D)                                                                                        \
    case D:                                                                                                     \
        if (which == 0) hipLaunchKernelGGL((attn_fwd_kernel<CT, D>), grid, block, 0, s, g);                     \
        else if (which == 1) hipLaunchKernelGGL((attn_bwd_dq_kernel<CT, D, false>), grid, block, 0, s, g);      \
        else if (which == 3) hipLaunchKernelGGL((attn_bwd_dq_kernel<CT, D, true>), grid, block, 0, s, g);       \
        else hipLaunchKernelGGL((attn_bwd_dkv_kernel<CT, D>), grid, block, 0, s, g);                            \
        break;
    switch (dhp) {
        BPM_ATTN_CASE(32)
        BPM_ATTN_CASE(64)
        BPM_ATTN_CASE(128)
        BPM_ATTN_CASE(256)
        default: return BPM_ERR_ARG;
    }
#undef BPM_ATTN_CASE
    BPM_CHECK_LAUNCH();
    return 0;
}

// the per-key-mask kernels (which: 0 forward, 1 dQ, 2 dK / dV)
template <typename CT>
int dispatch_kmask(int which, int dhp, const AGroupK& g, int total, hipStream_t s) {
    dim3 grid(total), block(NTHREADS);
#define BPM_ATTN_KCASE(D)                                                                                       \
    case D:                                                                                                     \
        if (which == 0) hipLaunchKernelGGL((attn_fwd_kmask_kernel<CT, D>), grid, block, 0, s, g);               \
        else if (which == 1) hipLaunchKernelGGL((attn_bwd_dq_kmask_kernel<CT, D>), grid, block, 0, s, g);       \
        else hipLaunchKernelGGL((attn_bwd_dkv_kmask_kernel<CT, D>), grid, block, 0, s, g);                      \
        break;
    switch (dhp) {
        BPM_ATTN_KCASE(32)
        BPM_ATTN_KCASE(64)
        BPM_ATTN_KCASE(128)
        BPM_ATTN_KCASE(256)
        default: return BPM_ERR_ARG;
    }
#undef BPM_ATTN_KCASE
    BPM_CHECK_LAUNCH();
    return 0;
}

// host checks + argument block of one *_kmask launch (which: 0 forward, 1 dQ, 2 dK / dV); nothing is launched on an error
int fill_kmask(AGroupK& gk, int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* masks, int nprob, uint64_t seed, int* total,
               int which) {
    if (dtype != BPM_BF16 && dtype != BPM_F32) return BPM_ERR_ARG;
    if (!masks) return BPM_ERR_ARG;
    int rc = fill(gk.g, probs, nprob, which == 2, seed, total, which);
    if (rc) return rc;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        if (!q.Q || !q.K || !q.V || !q.O || !q.lse) return BPM_ERR_ARG;
        if (which != 0 && (!q.dO || !q.delta)) return BPM_ERR_ARG;
        if (which == 1 && !q.dQ) return BPM_ERR_ARG;
        if (which == 2 && (!q.dK || !q.dV)) return BPM_ERR_ARG;
        if (q.dS || q.Pd) return BPM_ERR_ARG;                    // the score-gradient export has no masked instantiation
        if (!masks[i].mask || masks[i].ldm < q.S) return BPM_ERR_ARG;
        gk.m[i].mask = masks[i].mask; gk.m[i].ldm = masks[i].ldm;
    }
    for (int i = nprob; i < BPM_MAX_GROUP; ++i) { gk.m[i].mask = nullptr; gk.m[i].ldm = 0; }
    return 0;
}

int attn_kmask(int which, int kind, int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* masks, int nprob, uint64_t seed,
               void* stream) {
    AGroupK gk;
    int total = 0;
    int rc = fill_kmask(gk, dtype, probs, masks, nprob, seed, &total, which);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    BpmProfScope prof(kind, s, 4.0 * useful_pair_flops(probs, nprob), attn_bytes(probs, nprob, dtype == BPM_BF16 ? 2 : 4, which));
    return dtype == BPM_BF16 ? dispatch_kmask<bf16_t>(which, probs[0].dhp, gk, total, s) : dispatch_kmask<float>(which, probs[0].dhp, gk, total, s);
}

// the additive-mask kernels (which: 0 forward, 1 dQ, 2 dK / dV)
template <typename CT>
int dispatch_amask(int which, int dhp, const AGroupA& g, int total, hipStream_t s) {
    dim3 grid(total), block(NTHREADS);
#define BPM_ATTN_ACASE(D)                                                                                       \
    case D:                                                                                                     \
        if (which == 0) hipLaunchKernelGGL((attn_amask_kernel<CT, D, 0>), grid, block, 0, s, g);                \
        else if (which == 1) hipLaunchKernelGGL((attn_amask_kernel<CT, D, 1>), grid, block, 0, s, g);           \
        else hipLaunchKernelGGL((attn_amask_kernel<CT, D, 2>), grid, block, 0, s, g);                           \
        break;
    switch (dhp) {
        BPM_ATTN_ACASE(32)
        BPM_ATTN_ACASE(64)
        BPM_ATTN_ACASE(128)
        BPM_ATTN_ACASE(256)
        default: return BPM_ERR_ARG;
    }
#undef BPM_ATTN_ACASE
    BPM_CHECK_LAUNCH();
    return 0;
}

// One additive mask as a kernel reads it: `transposed` false: (mask, ldm) against [T, S]; true: (maskT, ldt) against [S, T].
// The forward-oriented array must be there in every entry (it is the mask; maskT only restates it).  float4 reads: the
// base 16-byte aligned, the leading dimension a multiple of 4.
// A head stride (0: one image for all heads) keeps every head image under the same rules: a multiple of 4 elements, at
// least one image long, and within 31 bits (the kernels carry it as an int).
int amask_desc(AAdd& a, const bpm_attn_hmask& m, int T, int S, bool transposed) {
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

// host checks + argument block of one *_amask launch (which: 0 forward, 1 dQ, 2 dK / dV); nothing is launched on an error
int fill_amask(AGroupA& ga, int dtype, const bpm_attn_problem* probs, const bpm_attn_hmask* masks, int nprob, uint64_t seed, int* total,
               int which) {
    if (dtype != BPM_BF16 && dtype != BPM_F32) return BPM_ERR_ARG;
    if (!masks) return BPM_ERR_ARG;
    int rc = fill(ga.g, probs, nprob, which == 2, seed, total, which);
    if (rc) return rc;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        if (!q.Q || !q.K || !q.V || !q.O || !q.lse) return BPM_ERR_ARG;
        if (which != 0 && (!q.dO || !q.delta)) return BPM_ERR_ARG;
        if (which == 1 && !q.dQ) return BPM_ERR_ARG;
        if (which == 2 && (!q.dK || !q.dV)) return BPM_ERR_ARG;
        if (q.dS || q.Pd) return BPM_ERR_ARG;                    // the score-gradient export has no masked instantiation
        rc = amask_desc(ga.m[i], masks[i], q.T, q.S, which == 2);
        if (rc) return rc;
    }
    for (int i = nprob; i < BPM_MAX_GROUP; ++i) ga.m[i] = AAdd{nullptr, 0, 0};
    return 0;
}

int attn_amask(int which, int kind, int dtype, const bpm_attn_problem* probs, const bpm_attn_hmask* masks, int nprob, uint64_t seed,
               void* stream) {
    AGroupA ga;
    int total = 0;
    int rc = fill_amask(ga, dtype, probs, masks, nprob, seed, &total, which);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int sz = dtype == BPM_BF16 ? 2 : 4;
    double mbytes = 0;                                           // every head of a problem reads the whole mask once (L2 serves the repeats)
    for (int i = 0; i < nprob; ++i) mbytes += 4.0 * probs[i].T * probs[i].S;
    BpmProfScope prof(kind, s, 4.0 * useful_pair_flops(probs, nprob), attn_bytes(probs, nprob, sz, which) + mbytes);
    return dtype == BPM_BF16 ? dispatch_amask<bf16_t>(which, probs[0].dhp, ga, total, s) : dispatch_amask<float>(which, probs[0].dhp, ga, total, s);
}

// ---- bpm_attn_bwd_dbias: check / choose / fill / launch -----------------------------------------------------------------
// check: everything about the problems and the outputs that can be refused on the host; nothing is dereferenced
int dbias_check(const bpm_attn_problem* probs, const bpm_attn_dbias* outs, int nprob) {
    if (nprob < 1 || nprob > BPM_MAX_GROUP || !probs || !outs) return BPM_ERR_ARG;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        const bpm_attn_dbias& o = outs[i];
        if (q.B < 1 || q.H < 1 || q.T < 1 || q.S < 1 || q.dh < 1 || q.dh > q.dhp) return BPM_ERR_ARG;
        if (q.T > (1 << 22) || q.S > (1 << 22)) return BPM_ERR_ARG;      // index arithmetic is 32-bit, as in fill()
        if ((long)(q.T > q.S ? q.T : q.S) * q.dhp * 4 > (1l << 31)) return BPM_ERR_ARG;
        if (q.dhp != probs[0].dhp || (q.dhp != 32 && q.dhp != 64 && q.dhp != 128 && q.dhp != 256)) return BPM_ERR_ARG;
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
size_t dbias_choose(DChoice* ch, const bpm_attn_problem* probs, const bpm_attn_dbias* outs, int nprob) {
    long tiles = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        ch[i].nimg = outs[i].head_stride != 0 ? q.H : 1;
        ch[i].nterm = outs[i].head_stride != 0 ? q.B : q.B * q.H;
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

// fill: the two argument blocks (the mask descriptors are checked here, by the rule of the other *_amask entries)
int dbias_fill(DGroup& g, DSumGroup& sg, const DChoice* ch, const bpm_attn_problem* probs, const bpm_attn_hmask* masks,
               const bpm_attn_dbias* outs, int nprob, uint64_t seed, void* ws, long* total, long* sum_blocks) {
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
        const int rc = amask_desc(a, masks[i], q.T, q.S, false);
        if (rc) return rc;
        p.Q = (const char*)q.Q; p.K = (const char*)q.K; p.V = (const char*)q.V; p.dO = (const char*)q.dO;
        p.lse = q.lse; p.delta = q.delta;
        p.m = a.m; p.ldm = a.ld; p.mhs = a.hs;
        p.B = q.B; p.H = q.H; p.T = q.T; p.S = q.S;
        p.mask_off = (q.mask_off > 0 && q.mask_off < (1 << 29)) ? q.mask_off : (1 << 29);
        if (q.q_pos0 < 0 || q.q_stride < 0 || q.q_pos0 > (1 << 24) || q.q_stride > (1 << 24)) return BPM_ERR_ARG;
        p.qpos0 = q.q_pos0; p.qstride = q.q_stride > 0 ? q.q_stride : 1;
        if ((long)p.qpos0 + (long)(q.T - 1) * p.qstride > (1l << 28)) return BPM_ERR_ARG;
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
    *total = blk; *sum_blocks = sblk;
    return 0;
}

template <typename CT>
int dbias_launch(int dhp, const DGroup& g, long total, const DSumGroup& sg, long sum_blocks, hipStream_t s) {
    dim3 grid((unsigned)total), block(NTHREADS);
    switch (dhp) {
        case 32: hipLaunchKernelGGL((attn_dbias_kernel<CT, 32>), grid, block, 0, s, g); break;
        case 64: hipLaunchKernelGGL((attn_dbias_kernel<CT, 64>), grid, block, 0, s, g); break;
        case 128: hipLaunchKernelGGL((attn_dbias_kernel<CT, 128>), grid, block, 0, s, g); break;
        case 256: hipLaunchKernelGGL((attn_dbias_kernel<CT, 256>), grid, block, 0, s, g); break;
        default: return BPM_ERR_ARG;
    }
    BPM_CHECK_LAUNCH();
    if (sum_blocks > 0) {
        hipLaunchKernelGGL(attn_dbias_sum_kernel, dim3((unsigned)sum_blocks), block, 0, s, sg);
        BPM_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

extern "C" size_t bpm_attn_bwd_dbias_ws_bytes(const bpm_attn_problem* probs, const bpm_attn_dbias* outs, int nprob) {
    DChoice ch[BPM_MAX_GROUP];
    if (dbias_check(probs, outs, nprob)) return 0;
    return dbias_choose(ch, probs, outs, nprob);
}

// The gradient of an additive mask (a learned attention bias): see bpm_attn_dbias in include/bpmult_hip.h.
extern "C" int bpm_attn_bwd_dbias(int dtype, const bpm_attn_problem* probs, const bpm_attn_hmask* masks, const bpm_attn_dbias* outs,
                                  int nprob, uint64_t seed, void* ws, size_t ws_bytes, void* stream) {
    if (dtype != BPM_BF16 && dtype != BPM_F32) return BPM_ERR_ARG;
    if (!masks) return BPM_ERR_ARG;
    int rc = dbias_check(probs, outs, nprob);
    if (rc) return rc;
    DChoice ch[BPM_MAX_GROUP];
    const size_t need = dbias_choose(ch, probs, outs, nprob);
    if (need > 0 && (!ws || ws_bytes < need || ((uintptr_t)ws & 15))) return BPM_ERR_ARG;
    DGroup g;
    DSumGroup sg;
    long total = 0, sum_blocks = 0;
    rc = dbias_fill(g, sg, ch, probs, masks, outs, nprob, seed, ws, &total, &sum_blocks);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int sz = dtype == BPM_BF16 ? 2 : 4;
    double bytes = 0;                                            // Q, K, V, dO, lse, delta in; the mask in, dB out (partials: overhead)
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        bytes += (double)q.B * q.H * ((2.0 * q.T + 2.0 * q.S) * q.dh * sz + 2.0 * q.T * 4) + 4.0 * q.T * q.S * ch[i].nimg * 2;
    }
    BpmProfScope prof(BPM_K_ATTN_BWD_DBIAS, s, 4.0 * useful_pair_flops(probs, nprob), bytes);      // S and dP: two products
    return dtype == BPM_BF16 ? dbias_launch<bf16_t>(probs[0].dhp, g, total, sg, sum_blocks, s)
                             : dbias_launch<float>(probs[0].dhp, g, total, sg, sum_blocks, s);
}

#ifdef BPM_LAB
extern "C" int bpm_debug_attn_pair(int mask) {
    if (mask < 0 || mask > 7) return BPM_ERR_ARG;
    g_attn_pair = mask;
    return 0;
}
#endif

extern "C" int bpm_attn_fwd(int dtype, const bpm_attn_problem* probs, int nprob, uint64_t seed, void* stream) {
    AGroup g;
    int total = 0;
    int rc = fill(g, probs, nprob, 0, seed, &total, 0);
    if (rc) return rc;
    for (int i = 0; i < nprob; ++i)
        if (!probs[i].Q || !probs[i].K || !probs[i].V || !probs[i].O || !probs[i].lse) return BPM_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    BpmProfScope prof(BPM_K_ATTN_FWD, s, 4.0 * useful_pair_flops(probs, nprob), attn_bytes(probs, nprob, dtype == BPM_BF16 ? 2 : 4, 0));
    return dtype == BPM_BF16 ? dispatch<bf16_t>(0, probs[0].dhp, g, total, s) : dispatch<float>(0, probs[0].dhp, g, total, s);
}

// dQ first (it also produces delta), then dK/dV on the same stream.
// parts: 1 = dQ (+ delta), 2 = dK/dV (reads the delta a dQ pass wrote), 3 = both in that order
static int attn_bwd_parts(int dtype, const bpm_attn_problem* probs, int nprob, uint64_t seed, void* stream, int parts) {
    AGroup g;
    int total = 0;
    int rc = fill(g, probs, nprob, 0, seed, &total, 1);
    if (rc) return rc;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        if (!q.Q || !q.K || !q.V || !q.O || !q.lse || !q.dO || !q.delta) return BPM_ERR_ARG;
        if ((parts & 1) && !q.dQ) return BPM_ERR_ARG;
        if ((parts & 2) && (!q.dK || !q.dV)) return BPM_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    // algorithmic backward = dP, dQ (first kernel) + dV, dK (second): 4 * pairs * dh each; recomputing S is overhead
    const double w = 4.0 * useful_pair_flops(probs, nprob);
    if (parts & 1) {
        BpmProfScope prof(BPM_K_ATTN_BWD_DQ, s, w, attn_bytes(probs, nprob, dtype == BPM_BF16 ? 2 : 4, 1));
        bool xp = false;
        for (int i = 0; i < nprob; ++i) xp = xp || probs[i].dS != nullptr;
        const int which = xp ? 3 : 1;
        rc = dtype == BPM_BF16 ? dispatch<bf16_t>(which, probs[0].dhp, g, total, s) : dispatch<float>(which, probs[0].dhp, g, total, s);
        if (rc) return rc;
    }
    if (parts & 2) {
        rc = fill(g, probs, nprob, 1, seed, &total, 2);
        if (rc) return rc;
        BpmProfScope prof(BPM_K_ATTN_BWD_DKV, s, w, attn_bytes(probs, nprob, dtype == BPM_BF16 ? 2 : 4, 2));
        rc = dtype == BPM_BF16 ? dispatch<bf16_t>(2, probs[0].dhp, g, total, s) : dispatch<float>(2, probs[0].dhp, g, total, s);
    }
    return rc;
}

extern "C" int bpm_attn_bwd(int dtype, const bpm_attn_problem* probs, int nprob, uint64_t seed, void* stream) {
    return attn_bwd_parts(dtype, probs, nprob, seed, stream, 3);
}
extern "C" int bpm_attn_bwd_dq(int dtype, const bpm_attn_problem* probs, int nprob, uint64_t seed, void* stream) {
    return attn_bwd_parts(dtype, probs, nprob, seed, stream, 1);
}
extern "C" int bpm_attn_bwd_dkv(int dtype, const bpm_attn_problem* probs, int nprob, uint64_t seed, void* stream) {
    return attn_bwd_parts(dtype, probs, nprob, seed, stream, 2);
}

// Attention with a per-key padding mask (HF's attention_mask): see bpm_attn_kmask in include/bpmult_hip.h.  The work
// tallied for the launch profiler is that of the unmasked problem (the mask lives on the device).
extern "C" int bpm_attn_fwd_kmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_kmask(0, BPM_K_ATTN_FWD, dtype, probs, masks, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dq_kmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_kmask(1, BPM_K_ATTN_BWD_DQ, dtype, probs, masks, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dkv_kmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_kmask(2, BPM_K_ATTN_BWD_DKV, dtype, probs, masks, nprob, seed, stream);
}

// Attention with an additive [T, S] mask (the reference's attn_mask argument): see bpm_attn_amask in include/bpmult_hip.h.
// The *_amask entries are the *_hmask entries at head stride 0: their masks are restated as bpm_attn_hmask on the host.
namespace {
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
extern "C" int bpm_attn_fwd_amask(int dtype, const bpm_attn_problem* probs, const bpm_attn_amask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_amask(0, BPM_K_ATTN_FWD, dtype, probs, HMasks(masks, nprob).p, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dq_amask(int dtype, const bpm_attn_problem* probs, const bpm_attn_amask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_amask(1, BPM_K_ATTN_BWD_DQ, dtype, probs, HMasks(masks, nprob).p, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dkv_amask(int dtype, const bpm_attn_problem* probs, const bpm_attn_amask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_amask(2, BPM_K_ATTN_BWD_DKV, dtype, probs, HMasks(masks, nprob).p, nprob, seed, stream);
}
// ... and with one mask image per head (a learned per-head bias): see bpm_attn_hmask
extern "C" int bpm_attn_fwd_hmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_hmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_amask(0, BPM_K_ATTN_FWD, dtype, probs, masks, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dq_hmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_hmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_amask(1, BPM_K_ATTN_BWD_DQ, dtype, probs, masks, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dkv_hmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_hmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_amask(2, BPM_K_ATTN_BWD_DKV, dtype, probs, masks, nprob, seed, stream);
}

// Head-averaged attention probabilities of finished forward passes (see attn_maps_kernel); masks: the additive masks of
// bpm_attn_maps_amask (read through their transposes), or nullptr.
static int attn_maps_impl(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_hmask* masks, bool with_masks, int nprob, void* stream) {
    if (nprob < 1 || nprob > BPM_MAX_GROUP || !probs) return BPM_ERR_ARG;
    if (dtype != BPM_BF16 && dtype != BPM_F32) return BPM_ERR_ARG;
    if (with_masks && !masks) return BPM_ERR_ARG;
    const int sz = dtype == BPM_BF16 ? 2 : 4;
    MGroupA ga;
    MGroup& g = ga.g;
    g.nprob = nprob;
    long blk = 0;
    double flops = 0, bytes = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_map_problem& q = probs[i];
        MProb& p = g.p[i];
        if (!q.Q || !q.K || !q.lse || !q.W) return BPM_ERR_ARG;
        if (q.B < 1 || q.H < 1 || q.T < 1 || q.S < 1 || q.dh < 1 || q.dh > q.dhp || q.ldw < q.S) return BPM_ERR_ARG;
        if (q.T > (1 << 22) || q.S > (1 << 22)) return BPM_ERR_ARG;      // index arithmetic is 32-bit (rows * 512 B per head fits 31 bits)
        if ((long)(q.T > q.S ? q.T : q.S) * q.dhp * 4 > (1l << 31)) return BPM_ERR_ARG;   // ... and rows * 1 KiB at head_dim 256 in f32
        if (q.dhp != probs[0].dhp) return BPM_ERR_ARG;
        if ((((uintptr_t)q.Q | (uintptr_t)q.K) & 15) != 0 || (((uintptr_t)q.lse | (uintptr_t)q.W) & 3) != 0) return BPM_ERR_ALIGN;
        if (q.q_pos0 < 0 || q.q_stride < 0 || q.q_pos0 > (1 << 24) || q.q_stride > (1 << 24)) return BPM_ERR_ARG;
        p.Q = (const char*)q.Q; p.K = (const char*)q.K; p.lse = q.lse; p.W = q.W; p.ldw = q.ldw;
        p.B = q.B; p.H = q.H; p.T = q.T; p.S = q.S;
        p.mask_off = (q.mask_off > 0 && q.mask_off < (1 << 29)) ? q.mask_off : (1 << 29);
        p.qpos0 = q.q_pos0; p.qstride = q.q_stride > 0 ? q.q_stride : 1;
        if ((long)p.qpos0 + (long)(q.T - 1) * p.qstride > (1l << 28)) return BPM_ERR_ARG;
        p.nqt = (q.T + MQT - 1) / MQT; p.nkt = (q.S + 63) / 64;
        p.blk0 = (int)blk;
        blk += (long)p.nqt * p.nkt * q.B;
        if (blk > (1l << 30)) return BPM_ERR_ARG;
        const double ts = (double)q.B * q.T * q.S;
        flops += 2.0 * ts * q.H * q.dh;
        bytes += (double)q.B * q.H * ((double)(q.T + q.S) * q.dh * sz + q.T * 4.0) + ts * 4.0;      // Q, K, lse in; W out
        if (with_masks) {
            const int rc = amask_desc(ga.m[i], masks[i], q.T, q.S, true);
            if (rc) return rc;
            bytes += 4.0 * q.T * q.S;
        }
    }
    for (int i = with_masks ? nprob : 0; i < BPM_MAX_GROUP; ++i) ga.m[i] = AAdd{nullptr, 0, 0};
    hipStream_t s = (hipStream_t)stream;
    BpmProfScope prof(BPM_K_ATTN_MAPS, s, flops, bytes);
    dim3 grid((unsigned)blk), block(NTHREADS);
    bool per_head = false;
    for (int i = 0; with_masks && i < nprob; ++i) per_head = per_head || ga.m[i].hs != 0;
#define BPM_MAPS_CASE(D)                                                                                         \
    case D:                                                                                                      \
        if (per_head) {                                                                                          \
            if (dtype == BPM_BF16) hipLaunchKernelGGL((attn_maps_kernel<bf16_t, D, true, true>), grid, block, 0, s, ga);   \
            else hipLaunchKernelGGL((attn_maps_kernel<float, D, true, true>), grid, block, 0, s, ga);            \
        } else if (with_masks) {                                                                                 \
            if (dtype == BPM_BF16) hipLaunchKernelGGL((attn_maps_kernel<bf16_t, D, true>), grid, block, 0, s, ga);   \
            else hipLaunchKernelGGL((attn_maps_kernel<float, D, true>), grid, block, 0, s, ga);                  \
        } else if (dtype == BPM_BF16) hipLaunchKernelGGL((attn_maps_kernel<bf16_t, D, false>), grid, block, 0, s, g);   \
        else hipLaunchKernelGGL((attn_maps_kernel<float, D, false>), grid, block, 0, s, g);                      \
        break;
    switch (probs[0].dhp) {
        BPM_MAPS_CASE(32)
        BPM_MAPS_CASE(64)
        BPM_MAPS_CASE(128)
        BPM_MAPS_CASE(256)
        default: return BPM_ERR_ARG;
    }
#undef BPM_MAPS_CASE
    BPM_CHECK_LAUNCH();
    return 0;
}

extern "C" int bpm_attn_maps(int dtype, const bpm_attn_map_problem* probs, int nprob, void* stream) {
    return attn_maps_impl(dtype, probs, nullptr, false, nprob, stream);
}
extern "C" int bpm_attn_maps_amask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_amask* masks, int nprob, void* stream) {
    return attn_maps_impl(dtype, probs, HMasks(masks, nprob).p, true, nprob, stream);
}
extern "C" int bpm_attn_maps_hmask(int dtype, const bpm_attn_map_problem* probs, const bpm_attn_hmask* masks, int nprob, void* stream) {
    return attn_maps_impl(dtype, probs, masks, true, nprob, stream);
}

// Fused crossmodal / self attention for BPMulT on gfx950: forward, dQ, dK/dV.
//
// Semantics (reference multihead_attention.py:86-130, transformer.py:209-216):
//   S = Qs K^T  (Qs already carries the dh^-0.5 scale, applied by the Q-projection epilogue)
//   key j visible to query i  iff  j - i < mask_off   (mask_off = 1 + |S-T|, or "infinite" without attn_mask)
//   P = softmax_fp32(S) over visible keys;  Pd = dropout(P);  O = Pd V
// No key-padding mask: zero-padded key rows take part.
// Two further visibility rules are separate instantiations of the same block bodies (a compile-time mask type; the kernels
// above never see them): the per-key byte mask of the *_kmask entries (KM) and the arbitrary additive fp32 [T, S] mask of
// the *_amask entries (AM: the reference's attn_mask argument as a tensor, multihead_attention.py:113-115), one image for
// all heads, or one per head through the *_hmask entries (a learned bias; its gradient is attn_dbias.hip); and both at once
// (AKAdd: the *_kamask entries, a key_padding_mask beside an attn_mask / attn_bias).
// This file: the three block bodies, their kernels and the forward / backward entries.  attn_maps.hip holds the
// head-averaged maps, attn_common.h what the three files share.
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
#include "attn_common.h"

namespace {

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
// M: the mask of the instantiation (NoMask, AMask, AAdd or AKAdd: both), mk its descriptor.
template <typename CT, int DHP, typename M>
BPM_DEV void attn_fwd_block(const AProb& P, const DropCfg& drop, char* smem, const int bh, const int qb, const M mk) {
    constexpr bool KM = has_bytes<M>, AM = has_add<M>;      // has a byte mask / has an additive image
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
        if constexpr (KM) { if (tid < KT && jm < P.S) n_vis = byte_of(mk).mask[(size_t)b * byte_of(mk).ldm + jm] != 0; }
    };
    if (ntile > 0) {
        kst.load(Kh, 0, P.S, tid); vst.load(Vh, 0, P.S, tid);
        if constexpr (KM) stage_mask(0);
    }
    const float* arow = nullptr;                       // AM: this lane's mask row
    if constexpr (AM) arow = image_of(add_of(mk), b, h) + (size_t)min(q, P.T - 1) * add_of(mk).ld;
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
template <typename CT, int DHP, bool XP, typename M>
BPM_DEV void attn_bwd_dq_block(const AProb& P, const DropCfg& drop, char* smem, const int bh, const int qb, const M mk) {
    constexpr bool KM = has_bytes<M>, AM = has_add<M>;      // has a byte mask / has an additive image
    static_assert(!XP || !KM, "the dS / Pd export would write over the byte mask that AKAdd carries in AProb::Pd (AGroupKA)");
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
        if constexpr (KM) { if (tid < C::KTQ && jm < P.S) n_vis = byte_of(mk).mask[(size_t)b * byte_of(mk).ldm + jm] != 0; }
    };
    if (ntile > 0) {
        kst.load(Kh, 0, P.S, tid); vst.load(Vh, 0, P.S, tid);
        if constexpr (KM) stage_mask(0);
    }
    const float* arow = nullptr;                       // AM: this lane's mask row
    if constexpr (AM) arow = image_of(add_of(mk), b, h) + (size_t)min(q, P.T - 1) * add_of(mk).ld;
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


// ---------------------------------------------------------------------------
// backward, dK and dV
// ---------------------------------------------------------------------------
// KM: per-key mask.  A lane owns one key: its byte is read once (never at j >= S); a hidden key sees no query row
// (ilo past every row), so its probabilities are exp2(-inf) = 0 and its dK / dV rows are exact zeros.  A block without
// any visible key skips its query tiles.
// AM: additive mask through its transpose (AAdd holds maskT [S, ldt]): the lane's key row, one float4 per 4 queries of a
// register group, never read at j >= S or at a group that starts at i >= T.  A -inf entry gives probability 0, so the
// pair adds exactly nothing to dK / dV.
template <typename CT, int DHP, typename M>
BPM_DEV void attn_bwd_dkv_block(const AProb& P, const DropCfg& drop, char* smem, const int bh, const int kb, const M mk) {
    constexpr bool KM = has_bytes<M>, AM = has_add<M>;      // has a byte mask / has an additive image
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
        if (j < P.S) kvis = byte_of(mk).mask[(size_t)b * byte_of(mk).ldm + j] != 0;
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
    if constexpr (AM) acol = image_of(add_of(mk), b, h) + (size_t)min(j, P.S - 1) * add_of(mk).ld;
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

// ---------------------------------------------------------------------------
// the kernels: eight wrappers of one schedule
// ---------------------------------------------------------------------------
// Kernel arguments: the unmasked kernels take AGroup and nothing else, the masked ones AGroup followed by one descriptor
// per problem (AMask: the *_kmask entries, AAdd: the *_amask / *_hmask entries; both: the *_kamask entries, AGroupKA
// below).  Named structs, not one template: a kernel's symbol spells its argument type, and the symbols are what
// profiles and tools know the kernels by.
struct AGroupK {
    AGroup g;
    AMask m[BPM_MAX_GROUP];
};
struct AGroupA {
    AGroup g;
    AAdd m[BPM_MAX_GROUP];
};
// Both masks (the *_kamask entries): AGroup and 18 x (AMask + AAdd) would be 4192 bytes, past the 4 KiB limit.  The masked
// entries refuse the dS / Pd export, so in this family those fields of AProb carry the byte mask instead (Pd: the bytes,
// xs_b: their leading dimension; dS stays NULL) -- set_byte_mask on the host, byte_mask_of in the kernel, nowhere else.
// A type of its own, so that the kernel's symbol and the launch dispatch tell the family from AGroupA.
struct AGroupKA : AGroupA {};
inline void set_byte_mask(AProb& p, const AMask& k) { p.dS = nullptr; p.Pd = (char*)k.mask; p.xs_b = k.ldm; }
BPM_DEV AMask byte_mask_of(const AProb& p) { return AMask{(const uint8_t*)p.Pd, p.xs_b}; }
// Per-sample images (the *_bmask / *_kbmask entries): AGroup and 18 x AAddB (24 bytes) are 3616 + 432 = 4048 bytes; the
// family with key bytes carries them in AProb as AGroupKA does.
struct AGroupB {
    AGroup g;
    AAddB m[BPM_MAX_GROUP];
};
struct AGroupKB : AGroupB {};
static_assert(sizeof(AGroupB) <= 4096, "kernel arguments are limited to 4 KiB");
static_assert(sizeof(AGroupKB) <= 4096, "kernel arguments are limited to 4 KiB");
static_assert(sizeof(AGroupK) <= 4096, "kernel arguments are limited to 4 KiB");
static_assert(sizeof(AGroupKA) <= 4096, "kernel arguments are limited to 4 KiB");
static_assert(sizeof(AGroupA) <= 4096, "kernel arguments are limited to 4 KiB");

// Every wrapper below: xcd_remap, pick the problem (and its mask), resolve dropout, pair the blocks, run the block body
// once or twice.  The schedule is spelled out in each: folding them into one function (or even one spelling of
// pick) moved instructions in 18 to 47 of the 80 instantiations, and these kernels are tuned to the register.
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
        attn_fwd_block<CT, DHP>(P, drop, smem, bh, pass ? second : first, NoMask{});
    }
}
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
        attn_bwd_dq_block<CT, DHP, XP>(P, drop, smem, bh, pass ? second : first, NoMask{});
    }
}
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
        attn_bwd_dkv_block<CT, DHP>(P, drop, smem, bh, pass ? second : first, NoMask{});
    }
}

// the same schedules with a per-key mask (bpm_attn_fwd_kmask / _bwd_dq_kmask / _bwd_dkv_kmask)
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
        attn_fwd_block<CT, DHP>(P, drop, smem, bh, pass ? second : first, km);
    }
}
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
        attn_bwd_dq_block<CT, DHP, false>(P, drop, smem, bh, pass ? second : first, km);
    }
}
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
        attn_bwd_dkv_block<CT, DHP>(P, drop, smem, bh, pass ? second : first, km);
    }
}

// ... and with an additive mask (bpm_attn_fwd_amask / _bwd_dq_amask / _bwd_dkv_amask and the *_hmask entries).
// Compiled for the occupancy of their unmasked siblings: the tile's mask values are 16 more live
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
        if constexpr (WHICH == 0) attn_fwd_block<CT, DHP>(P, drop, smem, bh, blk, am);
        else if constexpr (WHICH == 1) attn_bwd_dq_block<CT, DHP, false>(P, drop, smem, bh, blk, am);
        else attn_bwd_dkv_block<CT, DHP>(P, drop, smem, bh, blk, am);
    }
}

// ... and with both masks (bpm_attn_fwd_kamask / _bwd_dq_kamask / _bwd_dkv_kamask): the LDS of the *_kmask kernels (the
// tile's mask bytes behind the K / V images), the registers of the *_amask kernels plus the byte-mask staging.  Compiled
// for the occupancy of the *_amask sibling, one wave fewer where it would otherwise spill more than the sibling does: the
// dQ pass in bf16 at every head_dim (12 / 20 / 176 / 32 bytes per lane at 32 / 64 / 128 / 256 against 0 / 0 / 32 / 0) and
// in f32 at 128 (84 against 0), the bf16 forward at 256 (116 against 0).  What is left: DESIGN.md section 5.
template <typename CT>
constexpr int attn_waves_kam(int kernel, int dhp) {
    const bool bf = sizeof(CT) == 2;
    const bool lower = bf ? (kernel == 1 || (kernel == 0 && dhp == 256)) : (kernel == 1 && dhp == 128);
    return attn_waves_am<CT>(kernel, dhp) - (lower ? 1 : 0);
}

template <typename CT, int DHP, int WHICH>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(attn_waves_kam<CT>(WHICH, DHP), attn_waves_kam<CT>(WHICH, DHP)))) void attn_kamask_kernel(const AGroupKA ga) {
    typedef Cfg<CT, DHP> C;
    constexpr int ROWS = WHICH == 0 ? KT : WHICH == 1 ? C::KTQ : C::QTK;
    __shared__ __attribute__((aligned(16))) char smem[2 * ROWS * C::STRIDE + (WHICH == 2 ? 2 * C::QTK * 4 : ROWS)];
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = pick_index(ga.g, bid);
    const AProb& P = ga.g.p[pi];
    const AKAdd kam = AKAdd{byte_mask_of(P), ga.m[pi]};
    const DropCfg drop = bpm_resolve_drop(P.drop, ga.g.seedp);
    const int nb2 = P.pair ? (P.nblk + 1) >> 1 : P.nblk;
    const int bh = bid / nb2;
    const int first = (P.pair || WHICH == 2) ? bid % nb2 : P.nblk - 1 - bid % nb2, second = P.pair ? P.nblk - 1 - first : first;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass && second == first) break;
        const int blk = pass ? second : first;
        if constexpr (WHICH == 0) attn_fwd_block<CT, DHP>(P, drop, smem, bh, blk, kam);
        else if constexpr (WHICH == 1) attn_bwd_dq_block<CT, DHP, false>(P, drop, smem, bh, blk, kam);
        else attn_bwd_dkv_block<CT, DHP>(P, drop, smem, bh, blk, kam);
    }
}

// ... and the last two with one image per sample (bpm_attn_*_bmask / *_kbmask: AAddB, the image of (b, h) at
// m + b * bs + h * hs).  Instantiations of their own, so the kernels above keep their registers; the sample's offset is one
// more wave-uniform 64-bit product per block.  Compiled for the occupancy of the sibling above: no instantiation spills
// more than its sibling does (profiles/attn_bmask_resource_usage.txt).
template <typename CT, int DHP, int WHICH>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(attn_waves_am<CT>(WHICH, DHP), attn_waves_am<CT>(WHICH, DHP)))) void attn_bmask_kernel(const AGroupB ga) {
    typedef Cfg<CT, DHP> C;
    constexpr int ROWS = WHICH == 0 ? KT : WHICH == 1 ? C::KTQ : C::QTK;
    __shared__ __attribute__((aligned(16))) char smem[2 * ROWS * C::STRIDE + (WHICH == 2 ? 2 * C::QTK * 4 : 0)];
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = pick_index(ga.g, bid);
    const AProb& P = ga.g.p[pi];
    const AAddB am = ga.m[pi];
    const DropCfg drop = bpm_resolve_drop(P.drop, ga.g.seedp);
    const int nb2 = P.pair ? (P.nblk + 1) >> 1 : P.nblk;
    const int bh = bid / nb2;
    const int first = (P.pair || WHICH == 2) ? bid % nb2 : P.nblk - 1 - bid % nb2, second = P.pair ? P.nblk - 1 - first : first;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass && second == first) break;
        const int blk = pass ? second : first;
        if constexpr (WHICH == 0) attn_fwd_block<CT, DHP>(P, drop, smem, bh, blk, am);
        else if constexpr (WHICH == 1) attn_bwd_dq_block<CT, DHP, false>(P, drop, smem, bh, blk, am);
        else attn_bwd_dkv_block<CT, DHP>(P, drop, smem, bh, blk, am);
    }
}
template <typename CT, int DHP, int WHICH>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(attn_waves_kam<CT>(WHICH, DHP), attn_waves_kam<CT>(WHICH, DHP)))) void attn_kbmask_kernel(const AGroupKB ga) {
    typedef Cfg<CT, DHP> C;
    constexpr int ROWS = WHICH == 0 ? KT : WHICH == 1 ? C::KTQ : C::QTK;
    __shared__ __attribute__((aligned(16))) char smem[2 * ROWS * C::STRIDE + (WHICH == 2 ? 2 * C::QTK * 4 : ROWS)];
    if (BPM_BASE_PRIO) __builtin_amdgcn_s_setprio(BPM_BASE_PRIO);
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int pi = pick_index(ga.g, bid);
    const AProb& P = ga.g.p[pi];
    const AKAddB kam = AKAddB{byte_mask_of(P), ga.m[pi]};
    const DropCfg drop = bpm_resolve_drop(P.drop, ga.g.seedp);
    const int nb2 = P.pair ? (P.nblk + 1) >> 1 : P.nblk;
    const int bh = bid / nb2;
    const int first = (P.pair || WHICH == 2) ? bid % nb2 : P.nblk - 1 - bid % nb2, second = P.pair ? P.nblk - 1 - first : first;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass && second == first) break;
        const int blk = pass ? second : first;
        if constexpr (WHICH == 0) attn_fwd_block<CT, DHP>(P, drop, smem, bh, blk, kam);
        else if constexpr (WHICH == 1) attn_bwd_dq_block<CT, DHP, false>(P, drop, smem, bh, blk, kam);
        else attn_bwd_dkv_block<CT, DHP>(P, drop, smem, bh, blk, kam);
    }
}

// ---------------------------------------------------------------------------
// host side.  Every entry is check (attn_common.h) / fill / choose / launch.
// ---------------------------------------------------------------------------
// bit k: kernel k (forward, dQ, dK/dV) takes two 64-row blocks per workgroup.  A constant in the product library; a
// -DBPM_LAB build (tools/attn_lab.py, the block-pairing test) can switch it through bpm_debug_attn_pair.
#ifdef BPM_LAB
int g_attn_pair = 7;
#else
constexpr int g_attn_pair = 7;
#endif

// fill: the argument block of one launch of kernel `kernel` (0 forward, 1 dQ, 2 dK / dV: its blocks run over S, the
// others' over T), with the checks of the group and of each problem's geometry
int fill(AGroup& g, const bpm_attn_problem* probs, int nprob, uint64_t seed, int* total, int kernel) {
    if (!group_ok(probs, nprob)) return BPM_ERR_ARG;
    g.nprob = nprob;
    g.seedp = bpm_seed_ptr(seed);
    int blk = 0;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        AProb& p = g.p[i];
        if (!geometry_ok(q, probs[0].dhp)) return BPM_ERR_ARG;
        p.Q = (const char*)q.Q; p.K = (const char*)q.K; p.V = (const char*)q.V;
        p.O = (char*)q.O; p.ldo = q.ldo; p.lse = q.lse;
        p.dO = (const char*)q.dO; p.delta = q.delta;
        p.dQ = (char*)q.dQ; p.lddq = q.lddq; p.dK = (char*)q.dK; p.lddk = q.lddk; p.dV = (char*)q.dV; p.lddv = q.lddv;
        p.B = q.B; p.H = q.H; p.T = q.T; p.S = q.S; p.dh = q.dh;
        if (!positions(q, p)) return BPM_ERR_ARG;
        p.dq_scale = q.dq_scale;
        p.dS = (char*)q.dS; p.Pd = (char*)q.Pd; p.xs_b = q.xs_b; p.xs_h = q.xs_h; p.xs_q = q.xs_q;
        if (q.dS || q.Pd) {       // both, whole 4-key groups, 4-element-aligned rows that do not run into each other
            if (!q.dS || !q.Pd || (q.S & 3) || ((q.xs_b | q.xs_h | q.xs_q) & 3) || q.xs_b < 0 || q.xs_h < 0 || q.xs_q < q.S) return BPM_ERR_ARG;
            if ((((uintptr_t)q.dS | (uintptr_t)q.Pd) & 15) != 0) return BPM_ERR_ALIGN;
        }
        p.drop = bpm_make_drop(q.drop_p, seed, q.drop_site);
        p.nblk = ((kernel == 2 ? q.S : q.T) + 63) / 64;
        p.blk0 = blk;
        p.pair = (g_attn_pair >> kernel) & 1;
        blk += (p.pair ? (p.nblk + 1) >> 1 : p.nblk) * q.B * q.H;
    }
    *total = blk;
    return 0;
}

// the two mask arrays of a *_kamask entry as one argument of the shared shape (fill_masked / attn_masked)
struct KAMasks { const bpm_attn_kmask* k; const bpm_attn_hmask* a; };
struct KBMasks { const bpm_attn_kmask* k; const bpm_attn_bmask* a; };      // ... of a *_kbmask entry
inline bool masks_given(const KAMasks* m) { return m->k && m->a; }
inline bool masks_given(const KBMasks* m) { return m->k && m->a; }
inline bool masks_given(const void* m) { return m != nullptr; }

// fill of a masked launch (A: AGroupK with bpm_attn_kmask masks, AGroupA with bpm_attn_hmask masks, AGroupKA with both as
// KAMasks; which: 0 forward, 1 dQ, 2 dK / dV, which reads an additive mask through its transpose); nothing is launched on
// an error
template <typename A, typename MK>
int fill_masked(A& a, int dtype, const bpm_attn_problem* probs, const MK* masks, int nprob, uint64_t seed, int* total, int which) {
    if (!dtype_ok(dtype)) return BPM_ERR_ARG;
    if (!masks_given(masks)) return BPM_ERR_ARG;
    int rc = fill(a.g, probs, nprob, seed, total, which);
    if (rc) return rc;
    if (!pointers_ok(probs, nprob, which)) return BPM_ERR_ARG;
    for (int i = 0; i < nprob; ++i) {
        const bpm_attn_problem& q = probs[i];
        if (q.dS || q.Pd) return BPM_ERR_ARG;                    // the score-gradient export has no masked instantiation
        if constexpr (std::is_same_v<A, AGroupK>) {
            if ((rc = kmask_desc(a.m[i], masks[i], q.S)) != 0) return rc;
        } else if constexpr (std::is_same_v<A, AGroupKA>) {
            AMask k;
            if ((rc = kmask_desc(k, masks->k[i], q.S)) != 0) return rc;
            if ((rc = amask_desc(a.m[i], masks->a[i], q.T, q.S, which == 2)) != 0) return rc;
            set_byte_mask(a.g.p[i], k);
        } else if constexpr (std::is_same_v<A, AGroupKB>) {
            AMask k;
            if ((rc = kmask_desc(k, masks->k[i], q.S)) != 0) return rc;
            if ((rc = bmask_desc(a.m[i], masks->a[i], q.H, q.T, q.S, which == 2)) != 0) return rc;
            set_byte_mask(a.g.p[i], k);
        } else if constexpr (std::is_same_v<A, AGroupB>) {
            if ((rc = bmask_desc(a.m[i], masks[i], q.H, q.T, q.S, which == 2)) != 0) return rc;
        } else if ((rc = amask_desc(a.m[i], masks[i], q.T, q.S, which == 2)) != 0) return rc;
    }
    for (int i = nprob; i < BPM_MAX_GROUP; ++i) a.m[i] = {};
    return 0;
}

// choose: the dQ pass exports dS / Pd (the XP instantiation) when any problem of the group asks for them
bool dq_exports(const bpm_attn_problem* probs, int nprob) {
    bool xp = false;
    for (int i = 0; i < nprob; ++i) xp = xp || probs[i].dS != nullptr;
    return xp;
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

// launch: kernel `which` (0 forward, 1 dQ, 2 dK / dV; xp: the dQ pass exports) of the family that takes A
template <typename A, typename CT, int D, int WHICH, bool XP = false>
constexpr auto attn_kernel() {
    if constexpr (std::is_same_v<A, AGroupA>) return &attn_amask_kernel<CT, D, WHICH>;
    else if constexpr (std::is_same_v<A, AGroupKA>) return &attn_kamask_kernel<CT, D, WHICH>;
    else if constexpr (std::is_same_v<A, AGroupB>) return &attn_bmask_kernel<CT, D, WHICH>;
    else if constexpr (std::is_same_v<A, AGroupKB>) return &attn_kbmask_kernel<CT, D, WHICH>;
    else if constexpr (std::is_same_v<A, AGroupK>)
        return WHICH == 0 ? &attn_fwd_kmask_kernel<CT, D> : WHICH == 1 ? &attn_bwd_dq_kmask_kernel<CT, D> : &attn_bwd_dkv_kmask_kernel<CT, D>;
    else if constexpr (WHICH == 1) return &attn_bwd_dq_kernel<CT, D, XP>;
    else return WHICH == 0 ? &attn_fwd_kernel<CT, D> : &attn_bwd_dkv_kernel<CT, D>;
}
template <typename A>
int attn_launch(int which, bool xp, int dtype, int dhp, const A& a, int total, void* stream) {
    return with_ct(dtype, [&](auto ct) {
        return with_dhp(dhp, [&](auto d) {
            typedef decltype(ct) CT;
            constexpr int D = decltype(d)::value;
            if (which == 0) return launch<attn_kernel<A, CT, D, 0>()>(total, NTHREADS, stream, a);
            if (which == 2) return launch<attn_kernel<A, CT, D, 2>()>(total, NTHREADS, stream, a);
            return xp ? launch<attn_kernel<A, CT, D, 1, true>()>(total, NTHREADS, stream, a)
                      : launch<attn_kernel<A, CT, D, 1>()>(total, NTHREADS, stream, a);
        });
    });
}

// a masked entry.  The work tallied for the launch profiler is that of the unmasked problem (a per-key mask lives on the
// device), plus the bytes of an additive mask: every head of a problem reads the whole mask once (L2 serves the repeats)
template <typename A, typename MK>
int attn_masked(int which, int kind, int dtype, const bpm_attn_problem* probs, const MK* masks, int nprob, uint64_t seed, void* stream) {
    A a;
    int total = 0;
    int rc = fill_masked(a, dtype, probs, masks, nprob, seed, &total, which);
    if (rc) return rc;
    double mbytes = 0;
    if constexpr (std::is_same_v<A, AGroupB> || std::is_same_v<A, AGroupKB>) {      // one image per sample and / or head that has its own
        for (int i = 0; i < nprob; ++i)
            mbytes += 4.0 * probs[i].T * probs[i].S * (a.m[i].bs ? probs[i].B : 1) * (a.m[i].hs ? probs[i].H : 1);
    } else if constexpr (!std::is_same_v<A, AGroupK>)
        for (int i = 0; i < nprob; ++i) mbytes += 4.0 * probs[i].T * probs[i].S;
    BpmProfScope prof(kind, (hipStream_t)stream, 4.0 * useful_pair_flops(probs, nprob),
                      attn_bytes(probs, nprob, dtype == BPM_BF16 ? 2 : 4, which) + mbytes);
    return attn_launch(which, false, dtype, probs[0].dhp, a, total, stream);
}

// dQ first (it also produces delta), then dK/dV on the same stream.
// parts: 1 = dQ (+ delta), 2 = dK/dV (reads the delta a dQ pass wrote), 3 = both in that order
int attn_bwd_parts(int dtype, const bpm_attn_problem* probs, int nprob, uint64_t seed, void* stream, int parts) {
    AGroup g;
    int total = 0;
    int rc = fill(g, probs, nprob, seed, &total, 1);
    if (rc) return rc;
    if (!pointers_ok(probs, nprob, parts)) return BPM_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int sz = dtype == BPM_BF16 ? 2 : 4;
    // algorithmic backward = dP, dQ (first kernel) + dV, dK (second): 4 * pairs * dh each; recomputing S is overhead
    const double w = 4.0 * useful_pair_flops(probs, nprob);
    if (parts & 1) {
        BpmProfScope prof(BPM_K_ATTN_BWD_DQ, s, w, attn_bytes(probs, nprob, sz, 1));
        rc = attn_launch(1, dq_exports(probs, nprob), dtype, probs[0].dhp, g, total, stream);
        if (rc) return rc;
    }
    if (parts & 2) {
        rc = fill(g, probs, nprob, seed, &total, 2);
        if (rc) return rc;
        BpmProfScope prof(BPM_K_ATTN_BWD_DKV, s, w, attn_bytes(probs, nprob, sz, 2));
        rc = attn_launch(2, false, dtype, probs[0].dhp, g, total, stream);
    }
    return rc;
}

}  // namespace

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
    int rc = fill(g, probs, nprob, seed, &total, 0);
    if (rc) return rc;
    if (!pointers_ok(probs, nprob, 0)) return BPM_ERR_ARG;
    BpmProfScope prof(BPM_K_ATTN_FWD, (hipStream_t)stream, 4.0 * useful_pair_flops(probs, nprob), attn_bytes(probs, nprob, dtype == BPM_BF16 ? 2 : 4, 0));
    return attn_launch(0, false, dtype, probs[0].dhp, g, total, stream);
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

// Attention with a per-key padding mask (HF's attention_mask): see bpm_attn_kmask in include/bpmult_hip.h.
extern "C" int bpm_attn_fwd_kmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupK>(0, BPM_K_ATTN_FWD, dtype, probs, masks, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dq_kmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupK>(1, BPM_K_ATTN_BWD_DQ, dtype, probs, masks, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dkv_kmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupK>(2, BPM_K_ATTN_BWD_DKV, dtype, probs, masks, nprob, seed, stream);
}

// Attention with an additive [T, S] mask (the reference's attn_mask argument): see bpm_attn_amask in include/bpmult_hip.h.
// The *_amask entries are the *_hmask entries at head stride 0 (HMasks).
extern "C" int bpm_attn_fwd_amask(int dtype, const bpm_attn_problem* probs, const bpm_attn_amask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupA>(0, BPM_K_ATTN_FWD, dtype, probs, HMasks(masks, nprob).p, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dq_amask(int dtype, const bpm_attn_problem* probs, const bpm_attn_amask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupA>(1, BPM_K_ATTN_BWD_DQ, dtype, probs, HMasks(masks, nprob).p, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dkv_amask(int dtype, const bpm_attn_problem* probs, const bpm_attn_amask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupA>(2, BPM_K_ATTN_BWD_DKV, dtype, probs, HMasks(masks, nprob).p, nprob, seed, stream);
}
// ... and with one mask image per head (a learned per-head bias): see bpm_attn_hmask
extern "C" int bpm_attn_fwd_hmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_hmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupA>(0, BPM_K_ATTN_FWD, dtype, probs, masks, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dq_hmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_hmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupA>(1, BPM_K_ATTN_BWD_DQ, dtype, probs, masks, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dkv_hmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_hmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupA>(2, BPM_K_ATTN_BWD_DKV, dtype, probs, masks, nprob, seed, stream);
}

// Attention with a per-key padding mask AND an additive mask (one image or one per head): see bpm_attn_fwd_kamask in
// include/bpmult_hip.h.
extern "C" int bpm_attn_fwd_kamask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_hmask* masks, int nprob,
                                   uint64_t seed, void* stream) {
    const KAMasks m{kmasks, masks};
    return attn_masked<AGroupKA>(0, BPM_K_ATTN_FWD, dtype, probs, &m, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dq_kamask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_hmask* masks, int nprob,
                                      uint64_t seed, void* stream) {
    const KAMasks m{kmasks, masks};
    return attn_masked<AGroupKA>(1, BPM_K_ATTN_BWD_DQ, dtype, probs, &m, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dkv_kamask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_hmask* masks, int nprob,
                                       uint64_t seed, void* stream) {
    const KAMasks m{kmasks, masks};
    return attn_masked<AGroupKA>(2, BPM_K_ATTN_BWD_DKV, dtype, probs, &m, nprob, seed, stream);
}

// Attention with one additive image per sample (and per head): see bpm_attn_bmask in include/bpmult_hip.h.  Kernels of
// their own (attn_bmask_kernel / attn_kbmask_kernel); at batch stride 0 the bits of the *_hmask / *_kamask entries.
extern "C" int bpm_attn_fwd_bmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_bmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupB>(0, BPM_K_ATTN_FWD, dtype, probs, masks, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dq_bmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_bmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupB>(1, BPM_K_ATTN_BWD_DQ, dtype, probs, masks, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dkv_bmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_bmask* masks, int nprob, uint64_t seed, void* stream) {
    return attn_masked<AGroupB>(2, BPM_K_ATTN_BWD_DKV, dtype, probs, masks, nprob, seed, stream);
}
extern "C" int bpm_attn_fwd_kbmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_bmask* masks, int nprob,
                                   uint64_t seed, void* stream) {
    const KBMasks m{kmasks, masks};
    return attn_masked<AGroupKB>(0, BPM_K_ATTN_FWD, dtype, probs, &m, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dq_kbmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_bmask* masks, int nprob,
                                      uint64_t seed, void* stream) {
    const KBMasks m{kmasks, masks};
    return attn_masked<AGroupKB>(1, BPM_K_ATTN_BWD_DQ, dtype, probs, &m, nprob, seed, stream);
}
extern "C" int bpm_attn_bwd_dkv_kbmask(int dtype, const bpm_attn_problem* probs, const bpm_attn_kmask* kmasks, const bpm_attn_bmask* masks, int nprob,
                                       uint64_t seed, void* stream) {
    const KBMasks m{kmasks, masks};
    return attn_masked<AGroupKB>(2, BPM_K_ATTN_BWD_DKV, dtype, probs, &m, nprob, seed, stream);
}

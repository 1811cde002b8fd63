// The body of attn_dbias_kernel and attn_dbias_bmask_kernel (attn_dbias.hip), included into each (see attn_maps_body.inc:
// as a shared device function it moved registers in all 16 instantiations the entries had).
// In scope: CTX (the compute type, or WithBytes<compute type> for KB), DHP, and ga, the kernel's argument block.
    typedef typename CtOf<CTX>::type CT;
    constexpr bool KB = CtOf<CTX>::bytes, PS = std::is_same_v<std::decay_t<decltype(ga)>, DGroupB>;
    const auto& grp = dbias_group(ga);
    typedef Cfg<CT, DHP> C;
    typedef typename Tr<CT>::frag frag;
    __shared__ __attribute__((aligned(16))) char smem[2 * KT * C::STRIDE + (KB ? KT : 0)];
    char* kimg = smem;
    char* vimg = smem + KT * C::STRIDE;
    uint8_t* smask = (uint8_t*)(smem + 2 * KT * C::STRIDE);    // KB only

    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int pi = 0;
#pragma unroll 1
    for (int i = 1; i < grp.nprob; ++i)
        if (bid >= grp.p[i].blk0) pi = i;
    const auto& P = grp.p[pi];
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
    auto head_of = [&](int t) {                                              // term -> (b * H + h)
        if constexpr (PS) return img * P.imul + t * P.tmul;
        else return P.per_head ? t * P.H + img : t;
    };

    if (kt * KT < jend && t0 < t1) {                   // block-uniform: a tile the mask_off rule hides keeps its zeros
        RowStage<CT, DHP, KT> kst, vst;
        uint32_t n_vis = 0;                            // KB, threads < KT: the next head's visibility of key kt * KT + tid
        auto stage = [&](int t) {
            const size_t bh = (size_t)head_of(t);
            kst.load(P.K + bh * P.S * C::ROWB, kt * KT, P.S, tid);
            vst.load(P.V + bh * P.S * C::ROWB, kt * KT, P.S, tid);
            if constexpr (KB) {
                const int jm = kt * KT + tid;
                n_vis = 0;
                if (tid < KT && jm < P.S) n_vis = ga.k[pi].mask[(bh / P.H) * ga.k[pi].ldm + jm] != 0;
            }
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
            if constexpr (PS) arow += (size_t)(bh / P.H) * P.mbs;
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
            if constexpr (KB) { if (tid < KT) smask[tid] = (uint8_t)n_vis; }
            __syncthreads();
            if (t + 1 < t1) stage(t + 1);
            if constexpr (KB) {
                const uint32_t w = *(const uint32_t*)(smask + 4 * (lane & 15));
                if (__builtin_amdgcn_ballot_w64(w != 0u) == 0) continue;      // no visible key (the same in every wave)
            }
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
                if constexpr (KB) {
                    const uint32_t w = *(const uint32_t*)(smask + 16 * n + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) e4[r] = ((w >> (8 * r)) & 0xffu) ? e4[r] : -INFINITY;
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
        float* orow;
        if constexpr (PS) orow = P.out + (size_t)sp * P.osplit + (size_t)(img / P.odiv) * P.obs + (size_t)(img % P.odiv) * P.ohs + (size_t)q * P.ldo;
        else orow = P.out + (size_t)sp * P.osplit + (size_t)img * P.ohs + (size_t)q * P.ldo;
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

// The body of attn_maps_kernel and attn_maps_bmask_kernel (attn_maps.hip), included into each: one text, and the compiler
// sees each kernel as if it were spelled out (a shared device function moved registers in 13 of the 48 instantiations).
// In scope: CTX (the compute type, or WithBytes<compute type> for KB), DHP, AM, PH, and ga, the kernel's argument block.
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
        std::conditional_t<per_sample_group<std::decay_t<decltype(ga)>>, AAddB, AAdd> am = {};
        if constexpr (AM) am = map_add(ga, pi);
        auto load_mask = [&](int h) {
            const float* acol = image_of(am, b, h) + (size_t)min(j, P.S - 1) * am.ld;
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

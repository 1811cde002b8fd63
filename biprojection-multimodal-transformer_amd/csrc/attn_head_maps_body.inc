// The body of attn_head_maps_kernel and attn_head_maps_bmask_kernel (attn_maps.hip), included into each (see
// attn_maps_body.inc).  In scope: CTX (the compute type, or WithBytes<compute type> for KB), DHP, AM, and ga, the kernel's
// argument block.
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
            const auto am = ga.m[pi];
            const float* acol = image_of(am, b, h) + (size_t)min(j, P.S - 1) * am.ld;
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

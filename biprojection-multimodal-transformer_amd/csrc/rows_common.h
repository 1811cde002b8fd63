// What more than one family of row kernels uses (rows_pack.hip, rows_norm.hip, rows_elem.hip, adam.hip; bert_embed.hip
// takes put4): the grouped-launch argument, small device helpers, and the shared pieces of the ONE shape of an entry
// point -- check, fill, choose, launch: grp_begin, with_width, and launch / with_ct from bpm_launch.h (which the
// attention files share).  Every row-kernel entry is GROUPED: one
// launch serves up to BPM_MAX_GROUP independent problems (the encoders of one level run in lock-step), passed by value
// in the kernel-argument segment; a block finds its problem from a prefix table of block counts.
// Everything sits in the unnamed namespace, as the kernels of those files do: their symbols carry it.
#pragma once
#include <cmath>
#include <type_traits>

#include "bpm_common.h"
#include "bpm_launch.h"
#include "../../include/bpmult_hip.h"

namespace {
constexpr int NT = 256;

template <typename CT> BPM_DEV void put(void* p, size_t i, float v) { ((CT*)p)[i] = Tr<CT>::from_f(v); }
template <typename CT>
BPM_DEV void put4(void* p, size_t i, f32x4 v) {
    if constexpr (sizeof(CT) == 4) *(f32x4*)((float*)p + i) = v;
    else { bf16x4 o; o[0] = (bf16_t)v[0]; o[1] = (bf16_t)v[1]; o[2] = (bf16_t)v[2]; o[3] = (bf16_t)v[3]; *(bf16x4*)((bf16_t*)p + i) = o; }
}

inline unsigned blocks_for(size_t n, int per_block, unsigned cap) {
    size_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

template <typename P> struct Grp {
    const uint64_t* seedp;              // dropout seed read at execution time (BPM_SEED_INDIRECT), or nullptr
    int n;
    unsigned blk0[BPM_MAX_GROUP + 1];   // prefix of block counts
    P p[BPM_MAX_GROUP];
};

// block -> (problem index, block within problem, blocks of that problem)
template <typename P>
BPM_DEV const P& pick(const Grp<P>& g, unsigned& bid, unsigned& nblk) {
    int pi = 0;
#pragma unroll 1
    for (int i = 1; i < g.n; ++i)
        if (bid >= g.blk0[i]) pi = i;
    nblk = g.blk0[pi + 1] - g.blk0[pi];
    bid -= g.blk0[pi];
    return g.p[pi];
}

template <typename D>
BPM_DEV const D& find_desc(const D* __restrict__ tab, int ndesc, unsigned bid) {
    int lo = 0, hi = ndesc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].blk0 <= bid) lo = mid; else hi = mid - 1;
    }
    return tab[lo];
}

constexpr unsigned CAP = 2048;   // blocks per problem for grid-stride kernels

// Host side.  The prologue of every grouped entry: the null / count check and the header of the kernel argument.  What a
// problem must satisfy, and the copy of its fields, stay with the entry.
template <typename P, typename Q>
inline bool grp_begin(Grp<P>& g, const Q* q, int n, uint64_t seed = 0) {
    if (!q || n < 1 || n > BPM_MAX_GROUP) return false;
    g.n = n; g.blk0[0] = 0; g.seedp = bpm_seed_ptr(seed);
    return true;
}

// Register widths W the one-wave-per-row kernels are instantiated at, UNIT columns each: the lists decide which
// instantiations exist.
template <int UNIT, int... W> struct Widths {};
using VecWidths = Widths<256, 1, 2, 3, 4>;                    // NV of ln_*_vec_kernel and kv_source_*_kernel
using RowWidths = Widths<64, 1, 2, 5, 8, 12, 16, 24, 32>;     // NE of ln_fwd_kernel and ln_bwd_kernel
// f(std::integral_constant<int, W>()) for the first W of the list with span <= UNIT * W; BPM_ERR_ARG when none covers it
template <int UNIT, int... W, typename F>
inline int with_width(Widths<UNIT, W...>, int span, F&& f) {
    int rc = BPM_ERR_ARG;
    (void)((span <= UNIT * W && ((rc = f(std::integral_constant<int, W>())), true)) || ...);
    return rc;
}
}  // namespace

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

// Column sums without float atomics in TWO launches (deterministic mode: bpm_ln_bwd_det outside the vector kernels'
// workspace route, bpm_rows_cast_ws): the first launch's blocks store their partial rows -- block b, array a at
// part[(b * FIN_ARR + a) * ncol] -- with plain stores; this finishing launch runs one block per DISTINCT destination row,
// which walks the problems in problem order, adds the partial rows of every (problem, array) that sums into its row in
// block order, and makes one plain read-modify-write.  The kernel boundary orders the two; problems that share a row are
// served by one owner, so nothing depends on the other problems of the launch beyond that stated order.
constexpr int FIN_ARR = 3;
struct ColFin {
    int n, ncol, nown;                           // ncol: floats per partial row
    int cols[BPM_MAX_GROUP];                     // live columns of problem i (<= ncol)
    unsigned blk0[BPM_MAX_GROUP + 1];            // partial rows of problem i: blocks [blk0[i], blk0[i + 1])
    float* dst[BPM_MAX_GROUP][FIN_ARR];          // where array a of problem i is added, or null
    float* own[FIN_ARR * BPM_MAX_GROUP];         // the distinct destinations
};

inline void fin_begin(ColFin& f, int n, int ncol, const unsigned* blk0) {
    f.n = n; f.ncol = ncol; f.nown = 0;
    for (int i = 0; i <= n; ++i) f.blk0[i] = blk0[i];
    for (int i = 0; i < n; ++i) {
        f.cols[i] = ncol;
        for (int a = 0; a < FIN_ARR; ++a) f.dst[i][a] = nullptr;
    }
}

inline void fin_add(ColFin& f, int i, int a, float* dst) {
    f.dst[i][a] = dst;
    if (!dst) return;
    for (int k = 0; k < f.nown; ++k)
        if (f.own[k] == dst) return;
    f.own[f.nown++] = dst;
}

template <int ARRS>      // (a template: only the files that launch it emit it)
__global__ __launch_bounds__(256) void col_finish_kernel(const ColFin f, const float* part) {
    static_assert(ARRS == FIN_ARR, "one layout of the partial rows");
    float* dst = f.own[blockIdx.x];
    for (int i = 0; i < f.n; ++i)                         // problem order; a thread owns its columns throughout
        for (int a = 0; a < FIN_ARR; ++a) {
            if (f.dst[i][a] != dst) continue;             // block-uniform
            for (int c = threadIdx.x; c < f.cols[i]; c += 256) {
                float s = 0.f;
#pragma unroll 8
                for (unsigned b = f.blk0[i]; b < f.blk0[i + 1]; ++b) s += part[((size_t)b * FIN_ARR + a) * f.ncol + c];
                dst[c] += s;
            }
        }
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

/* bpmult_hip.h -- C ABI of libbpmult_hip.so, the MI355X (gfx950) implementation
 * of the BPMulT forward/backward hot path.
 *
 * The reference (Damorgal/Biprojection-Multimodal-Transformer) is pure Python:
 * its "FFI" for this path is the set of torch ops called by
 * bpmult/models/{mmtr,transformer,multihead_attention,position_embedding}.py.
 * Each entry point below replaces the ops named in its comment (file:line into
 * the reference); INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer owned by
 *    the caller (PyTorch allocates); nothing here allocates or frees;
 *  - every function returns 0 on success, BPM_ERR_* or a hipError_t otherwise
 *    (bpm_error_string() renders either); nothing is printed;
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it and
 *    the call returns without synchronising (graph-capturable);
 *  - `dtype` selects the compute type CT of MFMA operands: BPM_F32 (exact f32
 *    MFMA 16x16x4 -- parity mode) or BPM_BF16 (MFMA 16x16x32, f32 accumulate);
 *  - row-major CT buffers that feed a GEMM have a leading dimension that is a
 *    multiple of 32 elements and ZERO padding columns; residual-stream tensors
 *    are fp32 [(t*B + b), d] exactly as torch lays out [T,B,d];
 *  - dropout masks are a pure function of (seed, site, element index)
 *    (counter hash), so backward regenerates them; drop_p = 0 disables;
 *  - every `seed` argument is either a 63-bit value or BPM_SEED_INDIRECT |
 *    the address of a device uint64 that the kernels read WHEN THEY RUN: a
 *    launch sequence captured once into a hipGraph then replays with a fresh
 *    seed per step (the host stores it before each replay).  Both forms draw
 *    identical masks for the same seed value.
 */
#ifndef BPMULT_HIP_H
#define BPMULT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BPM_ABI_VERSION 5
#define BPM_SEED_INDIRECT (1ull << 63) /* seed = BPM_SEED_INDIRECT | (uintptr_t)device pointer to the uint64 seed */
#define BPM_MAX_GROUP 18 /* problems per grouped launch (6 encoders of a level x 3 projections) */
#define BPM_GEMM_MAX_GROUP 24 /* bpm_gemm_grouped alone: 6 encoders x (q, k, v, out) weight gradients in one launch */

enum { BPM_F32 = 0, BPM_BF16 = 1,
       BPM_BF16X3 = 2 /* bpm_gemm_grouped only: split-bf16 operands (bpm_split_rows), three bf16 MFMA products per fp32 product */ };
enum { BPM_ERR_ARG = -1, BPM_ERR_ALIGN = -2 };

int bpm_version(void);
const char* bpm_error_string(int code);

/* ------------------------------------------------------------------------
 * Grouped GEMM with fused epilogue.
 * Replaces: F.linear in MultiheadAttention._in_proj / out_proj
 * (multihead_attention.py:130,152-158), fc1/fc2 (transformer.py:186-190),
 * nn.Conv1d k=1 projections (mmtr.py:456-458,748-750), the GMU linears
 * (mmtr.py:189-195), the time-axis nn.Linear maps (mmtr.py:507-508) and the
 * corresponding autograd backward GEMMs (train.py:394).
 *   BPM_GEMM_NT: C[M,N] = A[M,K] . B[N,K]^T     (A, B k-contiguous)
 *   BPM_GEMM_NN: C[M,N] = A[M,K] . B[K,N]
 *   BPM_GEMM_TN: C[M,N] = A[K,M]^T . B[K,N]
 * v = ((acc + bias_n[n] + bias_m[m]) * alpha); ReLU; gate; dropout; + resid.
 * ---------------------------------------------------------------------- */
enum { BPM_GEMM_NT = 0, BPM_GEMM_NN = 1, BPM_GEMM_TN = 2 };
enum { BPM_OUT_F32 = 0, BPM_OUT_CT = 1, BPM_OUT_HEADS = 2 };
/* BPM_GEMM_KPAD_ZERO: the caller promises that every row of a k-contiguous operand (A of NT/NN, B of NT) is
 * readable up to its leading dimension and holds ZEROS in [K, ld) -- what every CT buffer written by this
 * library satisfies.  It lets the kernel use hardware-bounded buffer loads with no k-tail masking. */
/* BPM_GEMM_BACKGROUND: this product is off the caller's critical path (weight gradients, work put on a side
 * stream).  Forward / data-gradient products otherwise raise their waves' issue priority (s_setprio) so that, when
 * kernels of two streams share a CU, the critical-path kernel is served first. */
/* BPM_GEMM_A_OVERLAP / BPM_GEMM_B_OVERLAP: the rows of that operand OVERLAP in memory -- its leading dimension is
 * smaller than its row length (K of a k-contiguous operand, M / N of a k-strided one).  Row r is still the elements
 * [r*ld, r*ld + length): the sliding windows of a strided 1-D convolution over a channels-last signal are exactly such
 * a matrix (ld = stride*Cin, length = taps*Cin), so the convolution and its two gradients are products on the signal
 * itself and no window matrix is materialised (frontend.py; reference mmtr.py:93-108).  Needs BPM_GEMM_KPAD_ZERO
 * (hardware-bounded loads only: the operand must be readable up to (rows-1)*ld + length), and K % 64 == 0 when the
 * overlapping operand is k-contiguous (its k tail would otherwise read the next window's data instead of zeros). */
/* BPM_GEMM_CT_NARROW: a BPM_OUT_CT output writes its N columns only (by default the pad columns [N, ldc) of every row
 * receive zeros): for outputs whose rows are interleaved with other tensors' rows (ldc = several logical rows). */
enum { BPM_GEMM_ACCUM = 1, BPM_GEMM_RELU = 2, BPM_GEMM_ATOMIC = 4, BPM_GEMM_KPAD_ZERO = 8, BPM_GEMM_BACKGROUND = 16,
       BPM_GEMM_A_OVERLAP = 32, BPM_GEMM_B_OVERLAP = 64, BPM_GEMM_CT_NARROW = 128, BPM_GEMM_BATCHED = 256 };

typedef struct bpm_gemm_problem {
    const void* A;          /* CT */
    const void* B;          /* CT */
    void* C;                /* fp32 (BPM_OUT_F32) or CT */
    int M, N, K;
    int lda, ldb, ldc;      /* elements */
    const float* bias_n;    /* [N] or NULL */
    const float* bias_m;    /* [M] or NULL (time-axis Linear) */
    const float* resid;     /* fp32 [M, ldr] added after dropout, or NULL */
    int ldr;
    const void* gate;       /* CT [M, ldg]: v = gate > 0 ? v * gate_scale : 0 (ReLU+dropout backward), or NULL */
    int ldg;
    float gate_scale;
    float alpha;
    float drop_p;           /* dropout on element index m*N + n, keyed by (call seed, drop_site) */
    uint32_t drop_site;
    float* colsum;          /* [N] += column sums of v (before + resid), by atomics; or NULL (bias gradients) */
    int flags;              /* BPM_GEMM_* */
    int out_kind;           /* BPM_OUT_* */
    int splitk;             /* >1 needs BPM_GEMM_ATOMIC + BPM_OUT_F32 into a zeroed / accumulating buffer */
    /* BPM_OUT_HEADS: row m = t*B + b, column n = h*dh + c  ->  C[b][h][t][c] of [B,H,T,dhp] */
    int heads_B, heads_H, heads_T, heads_dh, heads_dhp;
    /* BPM_GEMM_TN only: colsum_a[m] += sum_k A[k, m] (the bias gradient that belongs to a weight gradient
     * dW = dY^T X: A = dY), taken from the operand tiles already in registers by one extra MFMA against a vector
     * of ones in the workgroups of the first N tile.  Needs splitk == 1.  NULL = off. */
    float* colsum_a;
    /* BPM_GEMM_BATCHED: `batch` products of this shape in one problem; operands / output of element i start
     * i * batch_stride_{a,b,c} elements behind the pointers above.  Plain stores (BPM_OUT_F32 / BPM_OUT_CT), no side
     * operands, N % 4 == 0; the 128 x 64 kernel only. */
    int batch, batch_stride_a, batch_stride_b, batch_stride_c;
} bpm_gemm_problem;

int bpm_gemm_grouped(int dtype, int variant, const bpm_gemm_problem* probs /* host */, int nprob,
                     uint64_t seed, void* stream);

/* ------------------------------------------------------------------------
 * Fused attention (never materialises the [T,S] scores).
 * Replaces: torch.bmm / += attn_mask / F.softmax(float) / F.dropout / torch.bmm
 * (multihead_attention.py:110-126), buffered_future_mask (transformer.py:209-216)
 * and their backward.  Q [B,H,T,dhp] (pre-scaled by dh^-0.5), K/V [B,H,S,dhp],
 * dO [B,H,T,dhp]: CT head-major, dhp in {32,64,128,256}.  O, dQ, dK, dV: CT
 * row-major [(t*B+b), ld], column h*dh + c.  lse, delta: fp32 [B,H,T].
 * mask_off: key j visible to query i iff j - i < mask_off (1 + |S-T| with
 * attn_mask; <= 0 means no mask).
 * ---------------------------------------------------------------------- */
typedef struct bpm_attn_problem {
    const void* Q; const void* K; const void* V;
    void* O; int ldo;
    float* lse;
    const void* dO;         /* backward only */
    float* delta;           /* backward scratch [B,H,T] */
    void* dQ; int lddq;     /* receives d(q before scaling) = dQs * dq_scale */
    void* dK; int lddk;
    void* dV; int lddv;
    int B, H, T, S, dh, dhp;
    int mask_off;
    float dq_scale;
    float drop_p;           /* on P, element index ((b*H+h)*T + i)*S + j, keyed by (call seed, drop_site) */
    uint32_t drop_site;
    int q_pos0, q_stride;   /* query row i is time step q_pos0 + i*q_stride for the mask rule (stride 0 = 1): a
                               gathered subset of query rows keeps its original visibility */
    /* bpm_attn_bwd_dq only, optional (both or neither; S % 4 == 0): dS = P o (drop o dP - delta), the gradient of the
     * scores, and Pd = drop o P, the probabilities after dropout, as CT elements at b*xs_b + h*xs_h + i*xs_q + j.  With a
     * handful of query rows dK = dS^T Q and dV = Pd^T dO have rank T per head and the caller may continue from these
     * [rows, S] matrices instead of bpm_attn_bwd_dkv (multihead_attention.py:110-130 backward). */
    void* dS; void* Pd;
    int xs_b, xs_h, xs_q;
} bpm_attn_problem;

int bpm_attn_fwd(int dtype, const bpm_attn_problem* probs /* host */, int nprob, uint64_t seed, void* stream);
int bpm_attn_bwd(int dtype, const bpm_attn_problem* probs /* host */, int nprob, uint64_t seed, void* stream);
/* The two halves of bpm_attn_bwd as separate launches: _dq writes dQ and delta = rowsum(dO * O); _dkv reads that
 * delta and writes dK, dV.  Only dQ is on the backward critical path (dK / dV feed weight gradients and the
 * key/value-source gradient), so the engine runs _dkv on its side stream. */
int bpm_attn_bwd_dq(int dtype, const bpm_attn_problem* probs /* host */, int nprob, uint64_t seed, void* stream);
int bpm_attn_bwd_dkv(int dtype, const bpm_attn_problem* probs /* host */, int nprob, uint64_t seed, void* stream);

/* The same three kernels with a PER-KEY PADDING MASK (HF BertSelfAttention's attention_mask, mmtr.py:144-158): one
 * bpm_attn_kmask per problem, a parallel host array.  mask: device bytes [B, ldm], ldm >= S; key j of sample b is visible
 * iff mask[b*ldm + j] != 0, AND visible under the problem's mask_off rule.  A hidden key gets probability exactly 0, adds
 * nothing to lse and receives exactly zero dK / dV rows; query rows are never masked (outputs at padded positions are
 * computed, as HF does).  The kernels never read `mask` at j >= S (tile padding is hidden without a load), so a tight
 * [B, S] tensor is legal.  EVERY SAMPLE MUST HAVE AT LEAST ONE VISIBLE KEY for each of its query rows -- not checked (it
 * would take a host sync); a row without one yields NaN.  A NULL mask or ldm < S is BPM_ERR_ARG; dS / Pd are not
 * supported here.  With an all-ones mask the results are bit-equal to the unmasked entries'. */
typedef struct bpm_attn_kmask {
    const uint8_t* mask;
    int ldm;
} bpm_attn_kmask;
int bpm_attn_fwd_kmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_kmask* masks /* host */, int nprob,
                       uint64_t seed, void* stream);
int bpm_attn_bwd_dq_kmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_kmask* masks /* host */, int nprob,
                          uint64_t seed, void* stream);
int bpm_attn_bwd_dkv_kmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_kmask* masks /* host */, int nprob,
                           uint64_t seed, void* stream);

/* Head-averaged attention maps of a finished forward pass: the reference's second return value
 * (multihead_attention.py:132-135, attn_weights.sum(dim=1) / num_heads), which the fused kernels never materialise.
 * Recomputed from the Q / K images and the lse that bpm_attn_fwd left:
 *   W[b][i][j] = (1/H) sum_h exp(Q[b,h,i,:] . K[b,h,j,:] - lse[b,h,i])   for a visible key, exactly 0.0f for a masked one
 * -- the softmax probabilities BEFORE attention dropout (what the reference returns in eval mode and with dropout 0).
 * Exponentials and the head sum in fp32; only [B,T,S] is written (columns S .. ldw-1 of a row are left untouched).
 * Q, K: 16-byte aligned; all problems of a launch share dhp. */
typedef struct bpm_attn_map_problem {
    const void* Q; const void* K;   /* CT, [B,H,T,dhp] (pre-scaled) / [B,H,S,dhp], as bpm_attn_problem */
    const float* lse;               /* [B,H,T], as written by bpm_attn_fwd */
    float* W; int ldw;              /* out: fp32 [B,T,ldw], ldw >= S */
    int B, H, T, S, dh, dhp;
    int mask_off;                   /* same visibility rule as bpm_attn_problem */
    int q_pos0, q_stride;
} bpm_attn_map_problem;

int bpm_attn_maps(int dtype, const bpm_attn_map_problem* probs /* host */, int nprob, void* stream);

/* The same kernels with an ARBITRARY ADDITIVE MASK (the reference's attn_mask argument, multihead_attention.py:113-115:
 * attn_weights += attn_mask.unsqueeze(0)): one bpm_attn_amask per problem, a parallel host array.  The score of
 * (query i, key j) is q_i . k_j + mask[i*ldm + j] in every one of the problem's B*H heads (Q pre-scaled as everywhere).
 * Entries are finite or -inf (+inf and NaN: undefined).  A -inf entry, or a key beyond the problem's mask_off limit (the
 * two rules are ANDed), gets probability exactly 0.0f, adds nothing to lse and contributes exactly nothing to dK / dV.
 * EVERY QUERY ROW MUST KEEP AT LEAST ONE VISIBLE KEY -- not checked; a row without one yields NaN, as in the reference.
 * These entries give the mask no gradient (bpm_attn_bwd_dbias below computes it).  Dropout indexes the probabilities as in
 * the other entries.
 *
 * Layout and reads.  mask: device fp32 [T, ldm], ldm >= S, ldm % 4 == 0, base 16-byte aligned (a lane of the forward /
 * dQ kernels reads the 4 consecutive keys of a register group as one 16-byte load).  The kernels read inside [T, ldm]
 * only, and whatever sits in columns S .. ldm-1 never reaches a result.
 * The dK / dV pass and the maps kernel hold one key per lane and walk query rows: they would read `mask` down a column.
 * Choice made here: the caller supplies the TRANSPOSE, maskT: device fp32 [S, ldt], maskT[j*ldt + i] == mask[i*ldm + j],
 * ldt >= T, ldt % 4 == 0, base 16-byte aligned, read the same way (columns T .. ldt-1 never reach a result).
 * bpm_attn_bwd_dkv_amask and bpm_attn_maps_amask require it; bpm_attn_fwd_amask and bpm_attn_bwd_dq_amask ignore it (NULL is
 * fine there).  The two arrays must agree -- not checked.
 * BPM_ERR_ARG, before anything is launched (and without a GPU): a NULL masks array or `mask`, ldm < S, a broken alignment
 * rule, a NULL / short / misaligned maskT where it is required, or dS / Pd set (no export here).
 * With an all-zeros mask the results are bit-equal to the unmasked entries'. */
typedef struct bpm_attn_amask {
    const float* mask;  int ldm;    /* fp32 [T, ldm], ldm >= S: added to score (i, j) */
    const float* maskT; int ldt;    /* its transpose, fp32 [S, ldt], ldt >= T: _bwd_dkv_amask and _maps_amask */
} bpm_attn_amask;
int bpm_attn_fwd_amask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_amask* masks /* host */, int nprob,
                       uint64_t seed, void* stream);
int bpm_attn_bwd_dq_amask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_amask* masks /* host */, int nprob,
                          uint64_t seed, void* stream);
int bpm_attn_bwd_dkv_amask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_amask* masks /* host */, int nprob,
                           uint64_t seed, void* stream);
/* bpm_attn_maps of forward passes that ran with these masks (lse from bpm_attn_fwd_amask): a -inf entry is exactly 0.0f. */
int bpm_attn_maps_amask(int dtype, const bpm_attn_map_problem* probs /* host */, const bpm_attn_amask* masks /* host */, int nprob,
                        void* stream);

/* PER-HEAD additive masks (a learned per-head attention bias): the four entries above with a head stride on the mask.
 * bpm_attn_hmask is bpm_attn_amask plus head_stride / head_strideT (elements, applied to mask / maskT): 0 means one
 * [T, ldm] image for all heads -- the *_amask entries, which are these entries at stride 0 (same kernels, same bits).
 * Otherwise head h of every sample reads the image at mask + h*head_stride (maskT + h*head_strideT): H images under the
 * layout and alignment rules above, each of them -- head_stride % 4 == 0, head_stride >= T*ldm (head_strideT >= S*ldt) and
 * below 2^31, or BPM_ERR_ARG.  Per-sample images: bpm_attn_bmask below.  The *_amask entries and their struct are unchanged, so
 * BPM_ABI_VERSION stays. */
typedef struct bpm_attn_hmask {
    const float* mask;  int ldm;    /* as bpm_attn_amask */
    const float* maskT; int ldt;
    int64_t head_stride, head_strideT;  /* elements between the images of consecutive heads; 0: one image for all heads */
} bpm_attn_hmask;
int bpm_attn_fwd_hmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_hmask* masks /* host */, int nprob,
                       uint64_t seed, void* stream);
int bpm_attn_bwd_dq_hmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_hmask* masks /* host */, int nprob,
                          uint64_t seed, void* stream);
int bpm_attn_bwd_dkv_hmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_hmask* masks /* host */, int nprob,
                           uint64_t seed, void* stream);
int bpm_attn_maps_hmask(int dtype, const bpm_attn_map_problem* probs /* host */, const bpm_attn_hmask* masks /* host */, int nprob,
                        void* stream);

/* The gradient of the additive mask (a learned attention bias): the gradient of the scores, which the fused kernels never
 * materialise, summed over the samples -- and over the heads when one image serves them all.
 *   dB[h*head_stride + i*lddb + j] = sum over b (and over h when head_stride == 0) of dS[b,h,i,j],
 *   dS = P o (drop o dP - delta), P = exp(q.k + mask - lse), dP = dO . V^T
 * in fp32.  Every (i, j) with i < T, j < S is written (a pair that a -inf entry or the mask_off rule hides: exactly 0.0f);
 * nothing is written at j >= S.  Reads Q, K, V, dO, lse and the delta that bpm_attn_bwd_dq[_amask] left: issue it after
 * that launch, as bpm_attn_bwd_dkv[_amask / _hmask].  Dropout draws the keep mask of the dQ pass (same hash, element index and
 * drop_site), so the dS summed here is the dS that pass multiplied by K.  `masks` are the forward pass's (only mask / ldm /
 * head_stride are read); head_stride of bpm_attn_dbias chooses the form of the RESULT independently of the mask's.
 * A workgroup owns a 64 x 64 tile of one output image and sums the heads that feed it in a fixed order; when the launch
 * would have fewer tiles than the chip holds workgroups at once, the head range of a tile is split over several workgroups,
 * whose fp32 partial images go through `ws` and are added in index order by a second kernel: the result is
 * bit-reproducible run to run (no float atomics).  bpm_attn_bwd_dbias_ws_bytes gives the workspace the same arrays
 * need (0: no split); ws is 16-byte aligned device memory, owned by the launch until it has run.
 * BPM_ERR_ARG, before anything is launched (and without a GPU): NULL arrays or pointers, lddb < S, lddb % 4 != 0, a
 * misaligned dB, a head_stride that is non-zero and smaller than T*lddb or no multiple of 4, a short or misaligned
 * workspace, dS / Pd set, problems of different dhp. */
typedef struct bpm_attn_dbias {
    float* dB; int lddb;            /* out: fp32 [T, lddb] (head_stride == 0) or H such images, lddb >= S, lddb % 4 == 0 */
    int64_t head_stride;            /* elements between the images of consecutive heads; 0: one image, summed over heads */
} bpm_attn_dbias;
size_t bpm_attn_bwd_dbias_ws_bytes(const bpm_attn_problem* probs /* host */, const bpm_attn_dbias* outs /* host */, int nprob);
int bpm_attn_bwd_dbias(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_hmask* masks /* host */,
                       const bpm_attn_dbias* outs /* host */, int nprob, uint64_t seed, void* ws, size_t ws_bytes, void* stream);

/* A PER-KEY PADDING MASK TOGETHER WITH AN ADDITIVE MASK (the reference's key_padding_mask beside its attn_mask, and a
 * learned attn_bias): the *_kamask entries take one bpm_attn_kmask AND one bpm_attn_hmask per problem, two parallel host
 * arrays.  Pair (sample b, head h, query i, key j) is visible iff all three rules say so: the problem's mask_off rule,
 * kmask[b*ldm + j] != 0, and mask[h*head_stride + i*ldm + j] > -inf; the score of a visible pair is
 * q_i . k_j + mask[h*head_stride + i*ldm + j].  A hidden pair behaves as in the two families: probability exactly 0.0f,
 * nothing added to lse, exactly nothing contributed to dK / dV (a key whose byte hides it for sample b gets exactly zero
 * dK / dV rows in that sample); a 64-key tile without a visible byte is skipped.  Query rows are never masked.
 * EVERY QUERY ROW OF EVERY SAMPLE MUST KEEP AT LEAST ONE VISIBLE KEY under the three rules together -- not checked (the
 * masks never travel to the host); a row without one yields NaN.
 * The byte mask is read as in the *_kmask entries (never at j >= S: a tight [B, S] tensor is legal), the additive image as
 * in the *_hmask entries (forward / dQ: mask; dK / dV and maps: maskT, required there).
 * BPM_ERR_ARG, before anything is launched (and without a GPU): the union of the two families' rules -- a NULL array of
 * either kind, a NULL byte mask or one with ldm < S, a NULL `mask`, ldm < S, ldm % 4 != 0 or a misaligned base of the
 * additive image, a NULL / short / misaligned maskT where it is required, a broken head-stride rule, dS / Pd set, problems
 * of different dhp.
 * With an all-ones byte mask the results are bit-equal to the *_hmask entries', with an all-zeros image to the *_kmask
 * entries'.
 * bpm_attn_maps_kmask: bpm_attn_maps of forward passes through bpm_attn_fwd_kmask; a key the byte mask hides is exactly
 * 0.0f in the map (all-ones: bit-equal to bpm_attn_maps).  bpm_attn_maps_kamask: the same after bpm_attn_fwd_kamask.
 * bpm_attn_bwd_dbias_kmask: bpm_attn_bwd_dbias after bpm_attn_bwd_dq_kamask; sample b contributes nothing at the keys
 * its byte mask hides (a key hidden in every sample: exactly 0.0f), same fixed summation order, no float atomics, same
 * workspace (bpm_attn_bwd_dbias_ws_bytes).  kmasks == NULL: bpm_attn_bwd_dbias itself, same kernels, same bits.
 * New entries only: BPM_ABI_VERSION stays. */
int bpm_attn_maps_kmask(int dtype, const bpm_attn_map_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */, int nprob,
                        void* stream);
int bpm_attn_fwd_kamask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */,
                        const bpm_attn_hmask* masks /* host */, int nprob, uint64_t seed, void* stream);
int bpm_attn_bwd_dq_kamask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */,
                           const bpm_attn_hmask* masks /* host */, int nprob, uint64_t seed, void* stream);
int bpm_attn_bwd_dkv_kamask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */,
                            const bpm_attn_hmask* masks /* host */, int nprob, uint64_t seed, void* stream);
int bpm_attn_maps_kamask(int dtype, const bpm_attn_map_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */,
                         const bpm_attn_hmask* masks /* host */, int nprob, void* stream);
int bpm_attn_bwd_dbias_kmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_hmask* masks /* host */,
                             const bpm_attn_kmask* kmasks /* host, or NULL */, const bpm_attn_dbias* outs /* host */, int nprob,
                             uint64_t seed, void* ws, size_t ws_bytes, void* stream);

/* PER-HEAD attention maps: the five bpm_attn_maps* entries without the head average,
 *   W[b][h][i][j] = exp(Q[b,h,i,:] . K[b,h,j,:] + mask - lse[b,h,i])   for a visible pair, exactly 0.0f for a hidden one
 * -- the [B*H, T, S] probabilities the reference forms before it averages them (multihead_attention.py:121), before
 * dropout.  Same arithmetic as the averaged kernel (the value written here is the addend that kernel sums for head h),
 * same masks under the same rules (the additive image is read through maskT), same mask_off / q_pos0 / q_stride.
 * bpm_attn_head_map_problem is bpm_attn_map_problem with W as fp32 [B, H, T, ldw] behind two strides in ELEMENTS:
 * the map of (sample b, head h) starts at W + b*batch_stride + h*head_stride, its row i at + i*ldw;
 * head_stride >= T*ldw and batch_stride >= H*head_stride.  Only W[b][h][i][0 .. S) is written: pad columns and any gap
 * between heads or samples are left untouched.  The output is H times the averaged one (B*H*T*S*4 bytes).
 * BPM_ERR_ARG, before anything is launched (and without a GPU): a NULL array or pointer, a geometry the averaged entries
 * refuse, ldw < S, a stride below its minimum, problems of different dhp, and the mask rules of the sibling entry;
 * BPM_ERR_ALIGN: Q / K not 16-byte aligned, lse / W not 4-byte aligned.  New entries only: BPM_ABI_VERSION stays. */
typedef struct bpm_attn_head_map_problem {
    const void* Q; const void* K;   /* as bpm_attn_map_problem */
    const float* lse;
    float* W; int ldw;              /* out: fp32 [B,H,T,ldw], ldw >= S */
    int B, H, T, S, dh, dhp;
    int mask_off;
    int q_pos0, q_stride;
    int64_t head_stride, batch_stride;  /* elements between the maps of consecutive heads / samples */
} bpm_attn_head_map_problem;
int bpm_attn_head_maps(int dtype, const bpm_attn_head_map_problem* probs /* host */, int nprob, void* stream);
int bpm_attn_head_maps_kmask(int dtype, const bpm_attn_head_map_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */,
                             int nprob, void* stream);
int bpm_attn_head_maps_amask(int dtype, const bpm_attn_head_map_problem* probs /* host */, const bpm_attn_amask* masks /* host */,
                             int nprob, void* stream);
int bpm_attn_head_maps_hmask(int dtype, const bpm_attn_head_map_problem* probs /* host */, const bpm_attn_hmask* masks /* host */,
                             int nprob, void* stream);
int bpm_attn_head_maps_kamask(int dtype, const bpm_attn_head_map_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */,
                              const bpm_attn_hmask* masks /* host */, int nprob, void* stream);

/* PER-SAMPLE additive masks and biases (torch.nn.MultiheadAttention's 3-D attn_mask [B*H, T, S], index b*H + h; a
 * cross-modal window or a time-distance bias over each sample's own time stamps): the *_hmask / *_kamask entries with a
 * sample stride on the image.  bpm_attn_bmask is bpm_attn_hmask plus batch_stride / batch_strideT (elements, applied to
 * mask / maskT).  Pair (sample b, head h, query i, key j) reads
 *   mask [b*batch_stride  + h*head_stride  + i*ldm + j]      (forward, dQ, the bias gradient)
 *   maskT[b*batch_strideT + h*head_strideT + j*ldt + i]      (dK / dV, both kinds of maps; required there)
 * so the four combinations of zero and non-zero strides are images of shape [T,S], [H,T,S], [B,1,T,S] and [B,H,T,S].
 * Every image obeys the layout and alignment rules of bpm_attn_amask (ldm >= S, ldm % 4 == 0, 16-byte aligned base, the
 * transpose likewise), every head stride the rules of bpm_attn_hmask, and a non-zero batch stride is a multiple of 4, at
 * least the images of one sample long (H*head_stride, or T*ldm when head_stride == 0; H*head_strideT or S*ldt for the
 * transpose) and below 2^31.  Visibility, exact zeros, mask_off / q_pos0 / q_stride and the dropout element index
 * ((b*H + h)*T + i)*S + j are those of the sibling entries, per image.
 * EVERY QUERY ROW OF EVERY SAMPLE MUST KEEP AT LEAST ONE VISIBLE KEY under all rules together -- not checked; a row
 * without one yields NaN.
 * The *_kbmask entries take the key-padding bytes of the *_kamask entries beside the images.
 * BPM_ERR_ARG, before anything is launched (and without a GPU): every rule of the *_hmask (*_kamask) sibling; a non-zero
 * batch stride that is no multiple of 4, smaller than the images of one sample, or >= 2^31; dS / Pd set.
 * Two bit-equalities: (1) at batch stride 0 every entry gives the bits of its *_hmask / *_kamask sibling, with and without
 * dropout; (2) a [B,H,T,S] image that repeats one [H,T,S] image in every sample gives the bits of the shared-image launch.
 * (The arithmetic of a sample does not depend on its neighbours: one launch over B samples equals B launches of one.)
 * Kernels of their own; the existing entries launch what they always did.  New entries only: BPM_ABI_VERSION stays. */
typedef struct bpm_attn_bmask {
    const float* mask;  int ldm;    /* as bpm_attn_hmask */
    const float* maskT; int ldt;
    int64_t head_stride,  head_strideT;
    int64_t batch_stride, batch_strideT;    /* elements between the images of consecutive samples; 0: the same image(s) for every sample */
} bpm_attn_bmask;
int bpm_attn_fwd_bmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_bmask* masks /* host */, int nprob,
                       uint64_t seed, void* stream);
int bpm_attn_bwd_dq_bmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_bmask* masks /* host */, int nprob,
                          uint64_t seed, void* stream);
int bpm_attn_bwd_dkv_bmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_bmask* masks /* host */, int nprob,
                           uint64_t seed, void* stream);
int bpm_attn_maps_bmask(int dtype, const bpm_attn_map_problem* probs /* host */, const bpm_attn_bmask* masks /* host */, int nprob,
                        void* stream);
int bpm_attn_head_maps_bmask(int dtype, const bpm_attn_head_map_problem* probs /* host */, const bpm_attn_bmask* masks /* host */,
                             int nprob, void* stream);
int bpm_attn_fwd_kbmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */,
                        const bpm_attn_bmask* masks /* host */, int nprob, uint64_t seed, void* stream);
int bpm_attn_bwd_dq_kbmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */,
                           const bpm_attn_bmask* masks /* host */, int nprob, uint64_t seed, void* stream);
int bpm_attn_bwd_dkv_kbmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */,
                            const bpm_attn_bmask* masks /* host */, int nprob, uint64_t seed, void* stream);
int bpm_attn_maps_kbmask(int dtype, const bpm_attn_map_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */,
                         const bpm_attn_bmask* masks /* host */, int nprob, void* stream);
int bpm_attn_head_maps_kbmask(int dtype, const bpm_attn_head_map_problem* probs /* host */, const bpm_attn_kmask* kmasks /* host */,
                              const bpm_attn_bmask* masks /* host */, int nprob, void* stream);

/* The bias gradient with a PER-SAMPLE RESULT: bpm_attn_bwd_dbias[_kmask] under per-sample masks, and with two strides on
 * the result, chosen independently of the mask's form:
 *   batch_stride != 0, head_stride != 0   dB[b*batch_stride + h*head_stride + i*lddb + j] = dS[b,h,i,j]        ([B,H,T,S])
 *   batch_stride != 0, head_stride == 0   dB[b*batch_stride + i*lddb + j] = sum over h of dS[b,h,i,j]           ([B,1,T,S])
 *   batch_stride == 0                      the two forms of bpm_attn_dbias ([H,T,S] / [T,S]), in their order of addition
 * A workgroup owns a 64 x 64 tile of one image and sums its terms in a fixed order (samples ascending, then heads); the
 * split through the workspace and the second kernel add in index order: no float atomics, bit-reproducible.
 * kmasks: the byte masks of a forward pass through bpm_attn_fwd_kbmask, or NULL.  At most BPM_MAX_GROUP problems.
 * BPM_ERR_ARG: the rules of bpm_attn_bwd_dbias_kmask and of bpm_attn_bmask, and for dB a non-zero batch_stride that is no
 * multiple of 4, smaller than one sample's images (H*head_stride, or T*lddb when head_stride == 0) or >= 2^31. */
typedef struct bpm_attn_dbias_b {
    float* dB; int lddb;            /* as bpm_attn_dbias */
    int64_t head_stride;
    int64_t batch_stride;           /* elements between the images of consecutive samples; 0: summed over the samples */
} bpm_attn_dbias_b;
size_t bpm_attn_bwd_dbias_bmask_ws_bytes(const bpm_attn_problem* probs /* host */, const bpm_attn_dbias_b* outs /* host */, int nprob);
int bpm_attn_bwd_dbias_bmask(int dtype, const bpm_attn_problem* probs /* host */, const bpm_attn_bmask* masks /* host */,
                             const bpm_attn_kmask* kmasks /* host, or NULL */, const bpm_attn_dbias_b* outs /* host */, int nprob,
                             uint64_t seed, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Row kernels.  All are grouped: `n` problems (<= BPM_MAX_GROUP) per launch,
 * problem arrays live in HOST memory and are copied into the kernel arguments.
 * ---------------------------------------------------------------------- */

/* Input staging.  Replaces x.transpose(1,2) / F.dropout on the text features /
 * .permute(2,0,1) around the Conv1d projections (mmtr.py:741-753): src fp32
 * [B,T,C] -> CT [(t*B+b), ld] (zero pad columns); backward: dsrc[b,t,c] =
 * drop_mult * g[(t*B+b), c]. */
typedef struct bpm_pack_problem {
    const float* src; void* dst;            /* forward */
    const float* g; int ldg; float* dsrc;   /* backward */
    int B, T, C, ld;
    float drop_p; uint32_t drop_site;       /* element index (b*T + t)*C + c */
} bpm_pack_problem;
int bpm_pack_rows_fwd(int dtype, const bpm_pack_problem* probs, int n, uint64_t seed, void* stream);
int bpm_pack_rows_bwd(const bpm_pack_problem* probs, int n, uint64_t seed, void* stream);

/* fp32 master weights -> CT shadows with zero-padded leading dimension; the
 * descriptor table lives in DEVICE memory (built once, reused every step).
 * Row r: dst[r*dst_ld + c] = c < cols ? src[r*src_ld + c] * (colscale ? colscale[c] : 1) : 0 for c < ld.
 * colscale (fp32 [cols], device) folds a LayerNorm gain into the projection that follows it: the key / value
 * side of a crossmodal layer normalises the SAME embedded source in every layer (transformer.py:167-172), so
 * the engine normalises it once without affine and uses W' = W * gamma, b' = W beta + b per layer. */
typedef struct bpm_pack_desc {
    const void* src;
    void* dst;
    int rows, cols, ld, src_ld, dst_ld;
    unsigned blk0;          /* first block of this tensor; a block covers 1024 (row, c<ld) elements */
    const float* colscale;
} bpm_pack_desc;
int bpm_pack_weights(int dtype, const bpm_pack_desc* table_dev, int ndesc, unsigned total_blocks, void* stream);

/* Folded bias of the above: out[n] = b[n] + sum_c W[n*ldw + c] * beta[c], n < rows.  Device-resident table;
 * one wave per output row, 4 rows per block (blk0 = first block of the entry). */
typedef struct bpm_fold_desc {
    const float* W; const float* beta; const float* b; float* out;
    int rows, cols, ldw;
    unsigned blk0;
} bpm_fold_desc;
int bpm_fold_bias(const bpm_fold_desc* table_dev, int ndesc, unsigned total_blocks, void* stream);

/* Backward of the folding.  The weight-gradient GEMM against the un-affined normalised source gives
 * dWf = dY^T xhat and the bias column sums give dbf; this turns them into the gradients of the real parameters:
 *   dW[n,c] += dWf[n,c]*gamma[c] + dbf[n]*beta[c];   dbias[n] += dbf[n];
 *   dgamma[c] += sum_n dWf[n,c]*W[n,c];               dbeta[c] += sum_n dbf[n]*W[n,c]      (atomics per block)
 * dWf is dense [rows, cols]; W / dW have row stride ldw.  16 rows per block. */
typedef struct bpm_unfold_desc {
    const float* dWf; const float* dbf; const float* W; const float* gamma; const float* beta;
    float* dW; float* dbias; float* dgamma; float* dbeta;
    int rows, cols, ldw;
    unsigned blk0;
} bpm_unfold_desc;
/* store_dw != 0: dW is WRITTEN (this launch is the first writer of those rows this step: no zero-fill, no read). */
int bpm_unfold_grads(const bpm_unfold_desc* table_dev, int ndesc, unsigned total_blocks, int store_dw, void* stream);
/* The same without float atomics (deterministic mode).  dW and dbias: the same bits as bpm_unfold_grads.  dgamma / dbeta:
 * every block stores its column sums as two partial rows in the workspace, and the block of a descriptor that finishes
 * last adds them in block order and makes one plain read-modify-write into dgamma / dbeta -- bitwise reproducible, the
 * same on the wide and the one-column path, and independent of the other descriptors of the launch.
 * max_cols >= the cols of every descriptor (a wider descriptor is not processed); descriptor i owns the blocks
 * [blk0, blk0 + ceil(rows / 16)).  ws: at least bpm_unfold_grads_ws_bytes(ndesc, total_blocks, max_cols) bytes, 16-byte
 * aligned, private to the stream for the duration of the launch (its ticket words are cleared by the entry, on the
 * stream, ahead of the kernel).  As with bpm_ln_bwd_ws the stream must OWN the dgamma / dbeta rows while the launch
 * runs, and two descriptors of one launch must not share them.  BPM_ERR_ARG: a NULL table or workspace, a workspace
 * that is misaligned or too small.  New entries only: BPM_ABI_VERSION stays. */
size_t bpm_unfold_grads_ws_bytes(int ndesc, unsigned total_blocks, int max_cols);
int bpm_unfold_grads_ws(const bpm_unfold_desc* table_dev, int ndesc, unsigned total_blocks, int store_dw, int max_cols,
                        void* ws, size_t ws_bytes, void* stream);

/* Zero a list of fp32 segments with one launch (device-resident table, built once).  A training step whose gradients
 * start from zero (zero_grad / `p.grad = None`, train.py:384-385,396-398) does not clear the whole flat gradient buffer:
 * the first weight-gradient GEMM of each large matrix stores instead of accumulating (no BPM_GEMM_ACCUM), and only
 * the small tensors that are summed from several launches (biases, LayerNorm affines, ...) are cleared by this.
 * blk0 = first block of the segment; a segment of n elements takes bpm_zero_segment_blocks(n) blocks. */
typedef struct bpm_zero_desc {
    float* p;
    unsigned n;
    unsigned blk0;
} bpm_zero_desc;
int bpm_zero_segment_blocks(unsigned n);
int bpm_zero_segments(const bpm_zero_desc* table_dev, int ndesc, unsigned total_blocks, void* stream);

/* Encoder prologue.  Replaces embed_scale * x + embed_positions(x[:,:,0]) and
 * F.dropout (transformer.py:66-79; position_embedding.py:8-27,62-76):
 * out = dropout(scale*x + table[pos]), pos = t+1 if x[t,b,0] != 0 else 0.
 * `table` is the fp32 sinusoid table [table_rows >= T+1, d] built on the host.
 * Backward: x = dy, out = dx, dx (+)= scale * drop_mult * dy. */
typedef struct bpm_embed_problem {
    const float* x; float* out;
    int T, B;
    int accumulate;                         /* backward only */
    float drop_p; uint32_t drop_site;       /* element index (t*B + b)*d + c */
    int pos0, pos_stride;                   /* row t is time step pos0 + t*pos_stride (stride 0 = 1): a gathered
                                               subset of rows keeps its original positions */
} bpm_embed_problem;
int bpm_embed_pos_fwd(const bpm_embed_problem* probs, int n, const float* table, int table_rows, int d,
                      float scale, uint64_t seed, void* stream);
int bpm_embed_pos_bwd(const bpm_embed_problem* probs, int n, int d, float scale, uint64_t seed, void* stream);

/* Key / value source of a crossmodal encoder, embedded and normalised in one pass (transformer.py:73-79 and the
 * affine-free half of the LayerNorm at transformer.py:167-172; the gain and bias are folded into the projections):
 *   forward   khat = LNhat(dropout_k(scale*xk + table[pos])), vhat likewise from xv with its own dropout site; CT
 *             [T*B, ld] with zero pad columns; mean / rstd [T*B] of both.  xk == xv (every call site of the model)
 *             is read once.  pos follows bpm_embed_pos_fwd.
 *   backward  dxk = scale * drop_k * dLNhat(gk), dxv likewise (gk / gv fp32 [T*B, d]; the embedded rows are recomputed
 *             from xk / xv, which must still hold the forward's values, with the forward's seed).  dxv == NULL or
 *             dxv == dxk: dxk receives the fp32 sum of the two instead.
 * Same bits as bpm_embed_pos_fwd -> bpm_ln_fwd (gamma 1, beta 0) and bpm_ln_bwd -> bpm_embed_pos_bwd on the same
 * inputs, without the four fp32 [T*B, d] tensors in between.
 * Domain (BPM_ERR_ARG outside it, nothing launched): d % 4 == 0, 4 <= d <= 1024, d <= ld <= 1024, ld % 4 == 0,
 * T*B*d < 2^32, table and every fp32 tensor 16-byte aligned, khat / vhat aligned to four CT elements,
 * table_rows >= pos0 + (T-1)*pos_stride + 2. */
typedef struct bpm_kv_source_problem {
    const float* xk; const float* xv;
    int T, B;
    int pos0, pos_stride;                   /* as in bpm_embed_problem */
    float drop_p_k; uint32_t drop_site_k;   /* element index (t*B + b)*d + c */
    float drop_p_v; uint32_t drop_site_v;
    void* khat; void* vhat; int ld;         /* forward outputs */
    float* mean_k; float* rstd_k; float* mean_v; float* rstd_v;   /* written by the forward, read by the backward */
    const float* gk; const float* gv;       /* backward inputs */
    float* dxk; float* dxv;                 /* backward outputs */
} bpm_kv_source_problem;
int bpm_kv_source_fwd(int dtype, const bpm_kv_source_problem* probs, int n, const float* table, int table_rows, int d,
                      float scale, float eps, uint64_t seed, void* stream);
int bpm_kv_source_bwd(const bpm_kv_source_problem* probs, int n, const float* table, int table_rows, int d, float scale,
                      uint64_t seed, void* stream);

/* LayerNorm (nn.LayerNorm(d), eps inside sqrt; transformer.py:91,153,167-172,
 * 183-185,227-229).  x fp32 [R,d].  Forward writes CT [R, ldo] with zero pad
 * columns, or plain fp32 [R, ldo] when out_f32; saves mean / rstd [R].
 * Backward: dx = add + dLN(dy); dgamma/dbeta += by atomics (both or neither).
 * Optional fused hand-off to the next backward GEMM (what bpm_rows_cast would
 * do with a = dx): cast = CT [R, ldc] copy of dx * dropout_mult(r*d + c) with
 * zero pad columns, cast_colsum[d] += its column sums (the bias gradient of
 * the linear whose output this residual branch was; transformer.py:174-175,
 * 189-190). */
typedef struct bpm_ln_problem {
    const float* x; const float* gamma; const float* beta;
    void* out; int ldo; int out_f32;
    float* mean; float* rstd;
    int R;
    const float* dy; int ldy; const float* add; float* dx; float* dgamma; float* dbeta;   /* backward */
    void* cast; int ldc; float* cast_colsum; float drop_p; uint32_t drop_site;           /* backward, optional */
} bpm_ln_problem;
int bpm_ln_fwd(int dtype, const bpm_ln_problem* probs, int n, int d, float eps, void* stream);
int bpm_ln_bwd(int dtype, const bpm_ln_problem* probs, int n, int d, uint64_t seed, void* stream);
/* Same with a caller-provided workspace of at least bpm_ln_bwd_ws_bytes(n, d) bytes (16-byte aligned, private to the
 * stream, ZERO when first used -- the library leaves its ticket words zero again): dgamma / dbeta / cast_colsum are then
 * produced from per-block partial rows by the last block of each problem to finish (single owner per column, fixed
 * order: bitwise reproducible) instead of float atomics from every block into the same rows.  ws == NULL: as bpm_ln_bwd.
 * The last block adds with a plain read-modify-write, so for the duration of the launch the stream must OWN those rows:
 * no other stream may accumulate into the same dgamma / dbeta / cast_colsum words concurrently (problems of one launch
 * that share a row are detected and fall back to atomics).  A launch that faults can leave ticket words non-zero:
 * re-zero (or re-create) the workspace after any error reported for its stream. */
size_t bpm_ln_bwd_ws_bytes(int n, int d);
int bpm_ln_bwd_ws(int dtype, const bpm_ln_problem* probs, int n, int d, uint64_t seed, void* ws, size_t ws_bytes, void* stream);
/* bpm_ln_bwd_ws for deterministic mode: the same launch, but a call whose dgamma / dbeta / cast_colsum would go out as
 * float atomics is computed without them: the vector kernels' workspace route where bpm_ln_bwd_ws takes it (the same
 * bits), and otherwise -- the scalar family (d % 4 != 0 or d > 1024), a misaligned row, problems of one launch that share
 * a gradient row -- the scalar kernel storing per-block partial rows, then a small finishing launch with one block per
 * distinct gradient row, which adds the partial rows in problem order, block order inside a problem, and makes one plain
 * read-modify-write (dx and the cast output: the bits of bpm_ln_bwd).  ws: at least bpm_ln_bwd_det_ws_bytes(n, d) bytes
 * serves either route (16-byte aligned, private to the stream, zero when first used); a missing, misaligned or too small
 * workspace is BPM_ERR_ARG and launches nothing -- never a fall-back to atomics.  The route is chosen for the whole
 * launch: a problem that alone takes the vector route is summed by the second route (256 blocks of 4 rows instead of 64
 * of 8) beside a problem that needs it, so its sums are independent of the other problems of a launch among launches
 * that take the same route (a fixed table gives the same bits on every run either way).  Rows that overlap without
 * being equal stay the caller's to avoid.  New entries only: BPM_ABI_VERSION stays. */
int bpm_ln_bwd_det(int dtype, const bpm_ln_problem* probs, int n, int d, uint64_t seed, void* ws, size_t ws_bytes, void* stream);
size_t bpm_ln_bwd_det_ws_bytes(int n, int d);

/* y = (a [+ b]) * dropout_mult(r*C + c); a is fp32 or (a_is_ct) CT.  Outputs,
 * each optional: CT copy [R, ldd] (pad zeroed), fp32 copy, column sums (+= by
 * atomics).  Residual-dropout backward + bias gradients (transformer.py:174-175,
 * 189-190), level 1->2 residual adds (mmtr.py:799-800). */
typedef struct bpm_cast_problem {
    const void* a; int lda; int a_is_ct;
    const float* b; int ldb;
    void* dst_ct; int ldd;
    int ct_cols;            /* CT columns written per row, [C, ct_cols) zeroed; 0 = ldd */
    float* dst_f32; int ldf;
    float* colsum;
    int R, C;
    float drop_p; uint32_t drop_site;
} bpm_cast_problem;
int bpm_rows_cast(int dtype, const bpm_cast_problem* probs, int n, uint64_t seed, void* stream);
/* bpm_rows_cast with its column sums computed without float atomics (deterministic mode), by either kernel of the
 * entry: every row block stores its partial row in the workspace, and a finishing launch adds them per distinct colsum
 * row in problem order, block order inside a problem, with one plain read-modify-write.  Every other output: the bits of
 * bpm_rows_cast.  ws: at least bpm_rows_cast_ws_bytes(probs, n) bytes, 16-byte aligned, private to the stream for the two
 * launches; BPM_ERR_ARG when it is NULL, misaligned or too small.  New entries only: BPM_ABI_VERSION stays. */
size_t bpm_rows_cast_ws_bytes(const bpm_cast_problem* probs, int n);
int bpm_rows_cast_ws(int dtype, const bpm_cast_problem* probs, int n, uint64_t seed, void* ws, size_t ws_bytes, void* stream);

/* Exact (erf) GELU, HF's hidden_act = "gelu" between intermediate.dense and output.dense (BertIntermediate):
 *   forward   g = 0.5 u (1 + erf(u / sqrt 2)),  u fp32 or (u_is_ct) CT [R, ldu];  g written as CT [R, ldg] with the pad
 *             columns [C, ldg) zeroed (the next GEMM's A operand under BPM_GEMM_KPAD_ZERO)
 *   backward  du = dg (Phi(u) + u phi(u)),  dg fp32 [R, lddg];  du written as CT [R, lddu], pad columns zeroed
 * All arithmetic in fp32, whole 4-element chunks: every leading dimension % 4 == 0 and >= C (a row's last chunk reads up to
 * 3 pad elements of its own input row), 4-element aligned pointers; C itself is arbitrary. */
typedef struct bpm_gelu_problem {
    const void* u; int ldu; int u_is_ct;
    void* g; int ldg;                       /* forward */
    const float* dg; int lddg;              /* backward */
    void* du; int lddu;
    int R, C;
} bpm_gelu_problem;
int bpm_gelu_fwd(int dtype, const bpm_gelu_problem* probs, int n, void* stream);
int bpm_gelu_bwd(int dtype, const bpm_gelu_problem* probs, int n, void* stream);

/* HF BertEmbeddings (absolute positions) in front of the text encoder's layer stack (mmtr.py:144-158), one problem per
 * launch.  ids / seg: int64 [B, L], batch-major as HF passes them (seg NULL = all zeros); word [V,d], pos [P,d] (L <= P),
 * type [Tt,d]: fp32 tables with contiguous rows.  Per time-major row r = t*B + b:
 *   s = (word[ids[b,t]] + type[seg[b,t]]) + pos[t]          (HF's summation order)
 *   x = (LN(s) * gamma + beta) * dropout_mult(r*d + c)      (eps inside the sqrt, biased variance)
 * Outputs: x fp32 [R,d]; optionally xc, the CT copy [R, ldc] of x with zero pad columns (bit-equal to what bpm_rows_cast
 * makes of x); s fp32 [R,d] and mean / rstd [R] of s for the backward.  The sum s is HF's two fp32 adds; the LayerNorm of a row is carried in fp64 registers and rounded once
 * to fp32 (x is the correctly rounded LayerNorm of s); nothing is bf16 whatever `dtype`, which
 * only names CT (BPM_F32 or BPM_BF16).  The kernel never reads outside a table: an id outside [0, V) or a type id outside
 * [0, Tt) contributes a ZERO row and adds one to the device counter *bad (one vector atomic; no host sync, no device
 * assert).  d % 32 == 0, 32 <= d <= 1024; tables, gamma, beta, x, s 16-byte aligned; B*L*d < 2^32.
 * BPM_ERR_ARG / BPM_ERR_ALIGN before anything is launched. */
typedef struct bpm_bert_embed_problem {
    const int64_t* ids; const int64_t* seg;
    const float* word; const float* pos; const float* type;
    int V, P, Tt;
    const float* gamma; const float* beta;
    int B, L;
    float* x;
    void* xc; int ldc;                      /* optional */
    float* s; float* mean; float* rstd;
    unsigned* bad;
    float drop_p; uint32_t drop_site;       /* element index (t*B + b)*d + c */
} bpm_bert_embed_problem;
int bpm_bert_embed_fwd(int dtype, const bpm_bert_embed_problem* prob /* host */, int d, float eps, uint64_t seed, void* stream);

/* Backward of the three gathers: ds fp32 [R,d] (time-major; the dx of bpm_ln_bwd_ws on (s, mean, rstd, gamma) with
 * dy = the layer stack's input gradient times the forward's dropout mask) -> the table gradients, each optional (NULL =
 * that table is frozen).  NO float atomics: every destination row is written by one owner that adds its rows in one
 * fixed order, so the result is bitwise reproducible.
 *   dword [V,d], ZEROED by the caller: sorted_ids / perm = the stable ascending sort of ids.view(-1) and its permutation
 *     (int64 [R], perm indexes the batch-major [B, L] ids).  Rows of one id are added in sorted order, runs longer than
 *     32 in 32-row pieces combined in order; ids outside [0, V) and row padding_idx (-1 = none) are skipped: those rows
 *     stay as the caller left them.
 *   dpos [P,d]: row t < L = sum_b ds[t*B + b]; rows >= L are not written.
 *   dtype [Tt,d]: every row written (two stages: per-block partial rows, then one owner per column); seg as in the forward.
 * ws: at least bpm_bert_embed_scatter_ws_bytes(B*L, d, Tt) bytes, 16-byte aligned, private to the stream for the call;
 * its contents do not matter.  Two launches.  Same limits on d as the forward. */
typedef struct bpm_bert_scatter_problem {
    const float* ds;
    const int64_t* sorted_ids; const int64_t* perm; const int64_t* seg;
    float* dword; float* dpos; float* dtype;
    int V, Tt, B, L;
    int64_t padding_idx;
    float* ws; size_t ws_bytes;
} bpm_bert_scatter_problem;
size_t bpm_bert_embed_scatter_ws_bytes(int rows, int d, int type_rows);
int bpm_bert_embed_scatter(const bpm_bert_scatter_problem* prob /* host */, int d, void* stream);

/* fp32 [R, C] (row stride ld) -> split bf16 [R, 2 ldp] for the BPM_BF16X3 products: columns [0, ldp) = hi = bf16(x),
 * columns [ldp, 2 ldp) = lo = bf16(x - hi), pad columns [C, ldp) of both planes zero (ldp % 4 == 0; the LDS-DMA GEMM
 * wants ldp % 128 == 0).  The parity-grade mode of the linear layers (multihead_attention.py:152-158,
 * transformer.py:186-190, F.linear everywhere on the path): x y ~ hi hi + hi lo + lo hi, f32 accumulation. */
typedef struct bpm_split_problem {
    const float* src; void* dst;
    int R, C, ld, ldp;
} bpm_split_problem;
int bpm_split_rows(const bpm_split_problem* probs, int n, void* stream);

/* Fusion-GMU gating (GatedMultimodalLayerFeatures.forward, mmtr.py:189-195):
 * out = z*tanh(a1)*x1 + (1-z)*tanh(a2)*x2, z = sigmoid(ag); a1,a2,ag fp32 [R,d]
 * are the three bias-free linears (GEMM outputs).  Backward writes da1,da2,dag
 * as CT [R, ldg] and the direct terms dx1 = dout*z*tanh(a1), dx2 likewise. */
typedef struct bpm_gmu_problem {
    const float* a1; const float* a2; const float* ag; const float* x1; const float* x2;
    float* out;
    const float* dout; void* da1; void* da2; void* dag; int ldg; float* dx1; float* dx2;   /* backward */
    int R;
} bpm_gmu_problem;
/* out = sum of n_in fp32 tensors of `count` elements each (16-byte aligned pointers; out may alias an input).  The autograd sums where one tensor feeds several consumers (mmtr.py:779-847: a level-1 output is a Fusion-GMU
 * operand twice and a level-2 key / value source; a projected input feeds up to eight encoders), grouped per launch. */
#define BPM_ADDN_MAX 8
typedef struct bpm_addn_problem {
    float* out;
    const float* src[8];    /* BPM_ADDN_MAX */
    int n_in;
    size_t count;
} bpm_addn_problem;
int bpm_add_n(const bpm_addn_problem* probs, int n, void* stream);

/* Head-major q / dO [B,H,T,dhp] (the attention operands) -> block rows [(h*T + t)*B + b, ld]: columns [h*dh, (h+1)*dh)
 * hold the head's vector, every other column zero -- the per-head products of the engine's low-rank key side (groups
 * with a handful of query rows) then are plain grouped GEMMs over all heads.  dbias (optional, [H*dh], WRITTEN):
 * sum_{b,t} rowsum(Pd[(h*T+t)*B+b, 0:S]) * dO[b,h,t,:], the value-projection bias gradient (column sums of
 * dV = Pd^T dO; multihead_attention.py:100-104 backward). */
typedef struct bpm_expand_problem {
    const void* q; const void* dO;      /* CT [B,H,T,dhp] */
    void* qexp; void* dOexp;            /* CT [H*T*B, ld] */
    const void* Pd;                     /* CT [H*T*B, S] (bpm_attn_problem.Pd with xs_h = T*B*S, xs_q = B*S, xs_b = S) or NULL */
    float* dbias;                       /* or NULL */
    int B, H, T, S, dh, dhp, ld;
} bpm_expand_problem;
int bpm_expand_heads(int dtype, const bpm_expand_problem* probs /* host */, int n, void* stream);

int bpm_gmu2_fwd(const bpm_gmu_problem* probs, int n, int d, void* stream);
int bpm_gmu2_bwd(int dtype, const bpm_gmu_problem* probs, int n, int d, void* stream);

/* Front-end: AudioEncoder of the 4-modal model (mmtr.py:93-108: Conv1d(96,96,k=128,stride 2) x 2 + AdaptiveAvgPool1d(200)).
 * A strided convolution over a channels-last signal xc[(b,pos), ci] is bpm_gemm_grouped on the signal itself, its rows
 * read overlapping (BPM_GEMM_A_OVERLAP / _B_OVERLAP; no window matrix):
 *   y[(b,l), co] = sum_{k,ci} Wr[co, k*Cin + ci] xc[(b, stride*l + k), ci] + bias     NT, lda = stride*Cin, K = taps*Cin
 *   dWr = dy^T . windows (TN, the signal as overlapping B; + colsum_a = bias gradient);   dx: the same NT form over the
 *   zero-padded dy, one problem per output phase pos % stride.
 * bpm_signal_pack:   out[r, c] (CT, leading dim ld, r < total_rows): row r = b*rows_per_batch + front + l, l < L, takes
 *                    x[b*sb + c*sc + l*sl] (fp32, element strides); every other row is zeros.  C % 4 == 0.
 * bpm_signal_unpack: x[b*sb + c*sc + l*sl] = l < Lvalid ? src[(b*rows_per_batch + l)*ld + c] : 0 for l < L (fp32 both).
 * bpm_adaptive_pool1d_*: torch.nn.AdaptiveAvgPool1d over the position axis of a fp32 [(b,l), C] matrix -> [(b,i), C]. */
int bpm_signal_pack(int dtype, const float* x, void* out, int B, int C, int L, int64_t sb, int64_t sc, int64_t sl,
                    int front, int rows_per_batch, int64_t total_rows, int ld, void* stream);
int bpm_signal_unpack(const float* src, float* x, int B, int C, int L, int64_t sb, int64_t sc, int64_t sl,
                      int Lvalid, int rows_per_batch, int ld, void* stream);
int bpm_adaptive_pool1d_fwd(const float* y, float* out, int B, int C, int Lin, int Lout, void* stream);
int bpm_adaptive_pool1d_bwd(const float* dout, float* dy, int B, int C, int Lin, int Lout, void* stream);

/* The [B,d]-sized tail (all fp32, exact f32 VALU arithmetic from the fp32 master weights):
 *   x_i   = (top_i + mid_i)[0] + (top_i + mid_i)[N_i - 1]            level 1 -> 3 residual + token pick, mmtr.py:806-808
 *           (i = l, v, a in the order of mmtr.py:857); x_3 = extra (poster projection, 4-modal, mmtr.py:574)
 *   z_i   = sigmoid(G_i [x_0|..|x_{n-1}]),  t_i = tanh(W_i x_i),  h = sum_i z_i t_i      TextShifting{3,4}Layer, mmtr.py:197-247
 *   p1    = dropout(relu(proj1 h)),  y = proj2 p1 + h,  logits = out_layer y            mmtr.py:577-583 / 860-866
 * top_i / mid_i are [N_i, B, d]; Wh[i] = gmu.hidden{i+1}.weight [d,d], Wg[i] = gmu.x{i+1}_gate.weight [d, n d].
 * The forward keeps x, z, t, h, p1, y ([B, n d] or [B, d]) for the backward; z is the model's gate output. */
typedef struct bpm_tail_desc {
    int B, d, n, C;
    int N[3];
    const float* top[3]; const float* mid[3];
    const float* extra;
    const float* Wh[4]; const float* Wg[4];
    const float* W1; const float* b1; const float* W2; const float* b2; const float* Wo; const float* bo;
    float out_dropout; uint32_t drop_site;
    float* x; float* z; float* t; float* h; float* p1; float* y; float* logits;
} bpm_tail_desc;
/* Backward: dlogits [B,C] (and optionally dz) in; parameter gradients are ACCUMULATED (+=) into dWh / dWg / dW1 / db1 / dW2 / db2 / dWo / dbo;
 * rows 0 and N_i - 1 of dtop[i] / dmid[i] ([N_i,B,d], the other rows are never touched: keep them zero) and dextra
 * [B,d] (NULL for n = 3) are WRITTEN; dy, dp1, dh [B,d] and dzp, dtp, dx [B, n d] are scratch. */
typedef struct bpm_tail_grads {
    const float* dlogits;
    const float* dz;        /* gradient of the returned gates z [B, n d], or NULL */
    float* dWh[4]; float* dWg[4];
    float* dW1; float* db1; float* dW2; float* db2; float* dWo; float* dbo;
    float* dtop[3]; float* dmid[3]; float* dextra;
    float* dy; float* dp1; float* dh; float* dzp; float* dtp; float* dx;
} bpm_tail_grads;
int bpm_tail_fwd(const bpm_tail_desc* t, uint64_t seed, void* stream);
int bpm_tail_bwd(const bpm_tail_desc* t, const bpm_tail_grads* g, void* stream);

/* Fused Adam step over ONE flat fp32 buffer (replaces torch.optim.Adam's per-tensor loop of
 * train.py:123-125,396-398 for the trunk, whose parameters / gradients are views into flat buffers).
 * torch.optim.Adam semantics (no amsgrad, L2 weight decay folded into the gradient); `step` is the 1-based step
 * count for the bias corrections; grad_scale multiplies the gradient first (1/world after an all-reduce sum);
 * zero_grad != 0 clears the gradient in the same pass.  n % 4 == 0, 16-byte aligned pointers. */
int bpm_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int step, float grad_scale, int zero_grad, void* stream);

/* The same step over the same flat buffers, table driven, WRITING THE CT WEIGHT SHADOWS as it stores the updated masters
 * (train.py:396-398 followed by the next forward's weight casts: one pass instead of two over the flat master).  The table
 * (device memory, built once) cuts the flat buffer into consecutive segments: off4 / n4 in units of 4 floats (16-byte
 * aligned), blk0 = first block (a segment takes bpm_adam_blocks(n4) blocks; entries sorted by blk0, covering the buffer).
 * dst != NULL: the segment starts with a whole [rows, cols] fp32 matrix (cols % 4 == 0) whose CT shadow is [rows, dst_ld];
 * shadow element (r, c) = CT(updated master (r, c)), pad columns are not touched.  dtype = the shadows' CT.
 * group: read by bpm_adam_step_groups only (below).  bpm_adam_step_table and bpm_adam_step_table_clip are entries into the
 * same kernel with one L2 group at the host's `step`; they ignore the word, whatever a caller's table holds there. */
typedef struct bpm_adam_seg {
    size_t off4;
    unsigned n4;
    unsigned blk0;
    void* dst;
    int rows, cols, dst_ld;
    int group;
} bpm_adam_seg;
int bpm_adam_blocks(size_t n4);
int bpm_adam_step_table(int dtype, const bpm_adam_seg* table_dev, int nseg, unsigned total_blocks, float* param, float* grad,
                        float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps, float weight_decay,
                        int step, float grad_scale, int zero_grad, void* stream);

/* Global gradient norm and clip coefficient, left ON THE DEVICE.  Together with bpm_adam_step_table_clip this replaces
 * torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm), which upstream MulT calls between backward() and
 * optimizer.step(): a foreach norm and a foreach multiply over ~1700 gradient views that read and then rewrite the whole
 * flat gradient buffer, and a host sync when the norm is logged.  Here the gradients are read once and not rewritten:
 * the optimizer kernel applies the coefficient as it reads them.
 * The table (device memory, built once) lists fp32 segments: p = first element (any 4-byte aligned address), n >= 1
 * elements, blk0 = first block; a segment takes bpm_grad_sumsq_blocks(p, n) blocks (it depends on p's offset inside its
 * 16-byte line), entries sorted by blk0.  ws: bpm_grad_sumsq_ws_bytes(total_blocks) bytes, 16-byte aligned, contents
 * irrelevant before and after (one partial sum per block; no state is kept between calls).  Two launches on `stream`.
 *   out[0] = total_norm = grad_scale * sqrt(sum of squares over the table + *extra_sumsq)
 *   out[1] = coef = min(1, max_norm / (total_norm + 1e-6))        (torch's formula; NaN propagates)
 * max_norm <= 0 or +inf: the norm only, coef = 1.  extra_sumsq: NULL, or a device float holding a sum of squares taken
 * elsewhere (parameters outside the flat buffer), added under the root.  out: 2 floats, 8-byte aligned.
 * Bitwise reproducible (no float atomics): <= 16 squares per lane and an 8-level tree per block in fp32, one partial per
 * block, the partials summed in a fixed order in fp64 -- relative error of the norm <= 13 * 2^-24 + one fp32 rounding. */
typedef struct bpm_sumsq_seg {
    const float* p;
    size_t n;
    unsigned blk0;
    unsigned pad_;
} bpm_sumsq_seg;
int bpm_grad_sumsq_blocks(const float* p, size_t n);
size_t bpm_grad_sumsq_ws_bytes(unsigned total_blocks);
int bpm_grad_sumsq(const bpm_sumsq_seg* table_dev, int nseg, unsigned total_blocks, float grad_scale, float max_norm,
                   const float* extra_sumsq, void* ws, size_t ws_bytes, float* out, void* stream);

/* bpm_adam_step_table with the gradient scale grad_scale * (*scale_dev): scale_dev is a device float written by an earlier
 * launch on the stream (out + 1 of bpm_grad_sumsq: the clip coefficient), read once per block.  scale_dev = NULL is
 * bpm_adam_step_table itself; *scale_dev == 1 gives bit-equal results. */
int bpm_adam_step_table_clip(int dtype, const bpm_adam_seg* table_dev, int nseg, unsigned total_blocks, float* param, float* grad,
                             float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps, float weight_decay,
                             int step, float grad_scale, const float* scale_dev, int zero_grad, void* stream);

/* The table-driven step with PARAMETER GROUPS, decoupled weight decay and a skip on a non-finite gradient norm: what
 * torch.optim.Adam(param_groups, decoupled_weight_decay=...) does for the trunk, and what torch.amp.GradScaler makes an
 * optimizer do when a gradient is inf / NaN.  Still one launch over the flat buffers that writes the CT shadows: THE
 * table-driven Adam kernel, which the two entries above launch as well.
 * Table: bpm_adam_seg as above, with seg.group = index into `groups` of the group the segment's parameters belong to (a
 * segment belongs to exactly one group), or -1: NOT STEPPED -- nothing of the segment is loaded and nothing stored (master,
 * moments and shadow keep their bits), except zeros to its gradients when zero_grad != 0 (a frozen parameter's slice is
 * still filled by the backward launches and must not grow for ever).  A group index >= ngroups is treated as -1.
 * groups: HOST array of ngroups (1 .. BPM_ADAM_MAX_GROUPS) entries, copied into the launch.  decoupled == 0: L2 decay,
 * g = grad * scale + weight_decay * p, the arithmetic of bpm_adam_step (one group 0 over the whole table is what
 * bpm_adam_step_table / _clip launch).  decoupled != 0: p *= 1 - lr * weight_decay first, then the Adam update on the
 * undecayed gradient (torch.optim.AdamW).  step: the group's 1-based step number for the bias corrections when steps_dev == NULL.
 * scale_dev: NULL or a device float multiplied into grad_scale (the clip coefficient, out + 1 of bpm_grad_sumsq).
 * norm_dev: NULL or a device float (out of bpm_grad_sumsq); when it is NaN or +-inf the step is SKIPPED: every block
 * stores nothing but the cleared gradients.  The decision is taken on the device; the host never waits.
 * steps_dev: NULL or int[ngroups] on the device, the groups' counts of APPLIED steps: the bias corrections then come from
 * steps_dev[group] + 1 (in double, as the host takes them) and groups[i].step is ignored; after the update a second tiny
 * launch adds one to every group's count -- or, when the step was skipped, adds one to *skipped_dev (NULL: not counted)
 * and leaves the counts alone.  Without steps_dev, skipped_dev is still advanced when norm_dev is given.
 * BPM_ERR_ARG: a NULL table / buffer / groups, ngroups outside 1..16, a host step < 1 when steps_dev == NULL;
 * BPM_ERR_ALIGN: the four buffers 16-byte, the device scalars 4-byte aligned.  Nothing is launched on an error. */
#define BPM_ADAM_MAX_GROUPS 16
typedef struct bpm_adam_group {
    float lr, beta1, beta2, eps, weight_decay;
    int decoupled;
    int step;
    int pad_;
} bpm_adam_group;
int bpm_adam_step_groups(int dtype, const bpm_adam_seg* table_dev, int nseg, unsigned total_blocks, float* param, float* grad,
                         float* exp_avg, float* exp_avg_sq, const bpm_adam_group* groups, int ngroups, float grad_scale,
                         const float* scale_dev, const float* norm_dev, int* steps_dev, int* skipped_dev, int zero_grad,
                         void* stream);

/* bpm_adam_step_groups over SEVERAL BUFFER SETS in one launch: a model whose parameters live in more than one flat store
 * (the trunk's and the text encoder's) is stepped by ONE kernel launch and ONE counter launch, so that every block of the
 * step reads the same steps_dev / norm_dev and the step counts advance once.  (Two bpm_adam_step_groups calls cannot
 * express this under steps_dev: the counts would advance between them.)
 * sets: 1 .. BPM_ADAM_MAX_SETS entries {param, grad, exp_avg, exp_avg_sq, n}: four flat fp32 buffers of n elements each
 * (n % 4 == 0, 16-byte aligned).  Table: bpm_adam_seg as above, except that
 *   seg.group = BPM_ADAM_SET_GROUP(set, group): the set the segment lies in (off4 / n4 are relative to that set's
 *               buffers) and its group, -1 (not stepped) included; only this entry reads the word that way;
 *   the segments need not cover a set, but their blocks are consecutive: seg[0].blk0 = 0, seg[i + 1].blk0 = seg[i].blk0 +
 *   bpm_adam_blocks(seg[i].n4), and total_blocks is their sum.
 * table_dev / sets_dev: the device-resident arrays the kernel reads (built once).  table_host / sets_host: the host arrays
 * they were uploaded from, with the same contents; EVERY check below reads these, so nothing waits for the device.
 * groups, grad_scale, scale_dev, norm_dev, steps_dev, skipped_dev, zero_grad and the shadow write: as bpm_adam_step_groups.
 * With one set whose table holds the same segments the results are bit-equal to bpm_adam_step_groups.
 * BPM_ERR_ARG: a NULL table / sets / groups (device or host copy), nsets outside 1..BPM_ADAM_MAX_SETS, a set with a NULL
 * buffer or n == 0 or n % 4 != 0, a segment whose set index is >= nsets, that reaches beyond its set, that is empty or
 * whose blk0 breaks the rule above, a shadow with cols % 4 != 0 or larger than its segment, ngroups outside 1..16, a host
 * step < 1 when steps_dev == NULL.  BPM_ERR_ALIGN: a buffer of a set not 16-byte, a device scalar not 4-byte aligned.
 * Nothing is launched on an error. */
#define BPM_ADAM_MAX_SETS 4
#define BPM_ADAM_SET_SHIFT 8
#define BPM_ADAM_SET_GROUP(set, group) ((int)(((unsigned)(set) << BPM_ADAM_SET_SHIFT) | ((unsigned)(group) & 0xffu)))
typedef struct bpm_adam_set {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    size_t n;
} bpm_adam_set;
int bpm_adam_step_sets(int dtype, const bpm_adam_seg* table_dev, const bpm_adam_seg* table_host, int nseg, unsigned total_blocks,
                       const bpm_adam_set* sets_dev, const bpm_adam_set* sets_host, int nsets, const bpm_adam_group* groups,
                       int ngroups, float grad_scale, const float* scale_dev, const float* norm_dev, int* steps_dev,
                       int* skipped_dev, int zero_grad, void* stream);

/* ------------------------------------------------------------------------
 * Training criterion.  Replaces nn.BCEWithLogitsLoss(pos_weight) / nn.CrossEntropyLoss(weight) / nn.L1Loss of
 * get_criterion (train.py:99-120) as called at train.py:333, and their autograd backward: the last torch compute ops of
 * the step BERT -> trunk -> loss -> Adam.  x = logits fp32 [B, ld >= C]; every element is carried in fp64 and rounded to
 * fp32 once, every sum is fp64 in one fixed order (no float atomics: loss and gradient are bitwise reproducible).
 *   BPM_LOSS_BCE  y fp32 [B, ldt >= C] (soft targets in [0, 1] are legal), weight = pos_weight [C] or NULL (= 1):
 *                 w = 1 + (pos_weight_c - 1) y;   l = (1 - y) x + w (max(-x, 0) + log1p(exp(-|x|)))
 *                 dl/dx = (1 - y) - w sigmoid(-x), sigmoid(-x) = (x >= 0 ? e : 1) / (1 + e), e = exp(-|x|);   mean: / (B C)
 *   BPM_LOSS_CE   t int64 [B], weight = class weight [C] or NULL (= 1).  Row i is KEPT when t_i != ignore_index and
 *                 0 <= t_i < C; every other row has loss 0, an all-zero gradient row and no part in the denominator.
 *                 m = max_c x_ic, S = sum_c exp(x_ic - m):   l_i = w[t_i] ((m - x_i[t_i]) + log S)
 *                 mean: / W, W = sum of w[t_i] over the kept rows (NaN when W = 0, as torch; sum is then 0)
 *                 dl/dx_ic = (exp(x_ic - m) / S - [c == t_i]) w[t_i] (/ W for mean).  C = 1: loss 0, gradient 0.
 *                 t_i is compared with [0, C) BEFORE any use as an index; an index that is neither ignore_index nor in
 *                 range adds one to *bad (int32 device counter, vector atomic add; NULL = not counted) and is treated
 *                 exactly like an ignored row: no device assert, no sync.
 *   BPM_LOSS_L1   y fp32 [B, ldt >= C]; l = |x - y|; dl/dx = sign(x - y) (exactly 0 where x == y); mean: / (B C); no weight.
 * loss: one fp32 for BPM_LOSS_MEAN / _SUM; dense [B, C] (BCE, L1) or [B] (CE) for BPM_LOSS_NONE.
 * dlogits_unit (optional, [B, ldd >= C]): the derivative of the REDUCED loss for an upstream gradient of 1 (so 1 / (B C)
 * or 1 / W is already in it); for BPM_LOSS_NONE the derivative of each element's / row's own loss.
 * Pad columns [C, ld) of logits / target are never read, those of dlogits_unit / dlogits never written.
 * ws: bpm_loss_ws_bytes(kind, reduction, B, C) bytes (0: may be NULL), 8-byte aligned, private to the stream for the
 * call; its contents do not matter before or after.  At most two launches.
 * BPM_ERR_ARG (nothing launched): NULL desc / logits / target / loss, B < 1, C < 1, unknown kind / reduction, ld < C,
 * ldt < C (BCE, L1), ldd < C with dlogits_unit, a weight for BPM_LOSS_L1, a workspace that is NULL or too small;
 * BPM_ERR_ALIGN: pointers not 4-byte (int64 target, ws: 8-byte) aligned.
 *
 * bpm_loss_bwd: dlogits[b, c] = dlogits_unit[b, c] * g, one launch; g is READ ON THE DEVICE when the kernel runs (what
 * (loss / gradient_accumulation_steps).backward() hands to the node, train.py:387-394): one fp32 for mean / sum (ldg
 * ignored), [B, ldg >= C] for none of BCE / L1, [B] for none of CE.  dlogits [B, lddl >= C] may alias dlogits_unit. */
enum { BPM_LOSS_BCE = 0, BPM_LOSS_CE = 1, BPM_LOSS_L1 = 2 };
enum { BPM_LOSS_MEAN = 0, BPM_LOSS_SUM = 1, BPM_LOSS_NONE = 2 };
typedef struct bpm_loss_desc {
    int kind, reduction;    /* BPM_LOSS_* */
    int B, C;
    const float* logits; int ld;
    const void* target; int ldt;
    const float* weight;
    int64_t ignore_index;   /* CE only */
    float* loss;
    float* dlogits_unit; int ldd;
    int* bad;               /* CE only, optional */
    void* ws; size_t ws_bytes;
} bpm_loss_desc;
size_t bpm_loss_ws_bytes(int kind, int reduction, int B, int C);
int bpm_loss_fwd(const bpm_loss_desc* d, void* stream);
int bpm_loss_bwd(const bpm_loss_desc* d, const float* g, int ldg, float* dlogits, int lddl, void* stream);

/* ------------------------------------------------------------------------
 * Evaluation of an epoch.  Replaces model_eval and weighted_acc (train.py:138-280): torch.sigmoid / softmax().argmax, the
 * loss.item() and three .cpu() copies of every batch, and scikit-learn's f1_score / accuracy_score /
 * average_precision_score at the end.  bpm_eval_update appends one batch to a store that the caller owns, in ONE launch
 * with no reduction and no host read; bpm_eval_finalize reduces the N stored rows to int64 counts and fp64 sums (five
 * launches and a memset for BPM_EVAL_MULTILABEL, two otherwise); the caller reads `result` and `counts` once.  Elements
 * are carried in fp64 and rounded once, floating-point sums are fp64 through one fixed tree, everything else is combined
 * in integers: no float atomics, two runs give identical bits.
 *
 * The store (rows [0, capacity), all allocated by the caller; only what the kind uses need be non-NULL):
 *   BPM_EVAL_MULTILABEL  logits fp32 [B, ld >= C], targets fp32 [B, ldt >= C].  score [cap, C] = (float) sigmoid((double) x);
 *                        pred [cap, C] bytes = score > 0.5f, compared ON THE FP32 SCORE as torch.sigmoid(out) > 0.5 is
 *                        (x = 0 and x = 1e-9 predict 0, x = 1e-6 predicts 1); label [cap, C] bytes = target == 1.  A target
 *                        that is neither 0 nor 1 is stored as label 0 and adds one to *bad.
 *   BPM_EVAL_REGRESSION  (cmu-mosi) C = 1: logits [B, ld >= 1], targets fp32 [B].  score [cap] = (float) sigmoid(x),
 *                        predict [cap] = score * 6 - 3 in two separately rounded fp32 operations (what numpy does to a
 *                        float32 array at train.py:261), raw [cap] = x, target [cap].
 *   BPM_EVAL_CLASSES     logits [B, ld >= C], targets int64 [B].  predict [cap] = argmax_c x[b, c] as fp32, the FIRST index
 *                        on ties; target [cap] as fp32; label [cap] bytes = 1 when the row takes part.  A class index
 *                        outside [0, C) is compared BEFORE any use, adds one to *bad, and its row is excluded from every
 *                        count and sum.  (The reference takes the argmax of the fp32 softmax, which can tie where the
 *                        logits do not: a departure.)
 * bad: int32 device counter (one vector atomic add per block; NULL = not counted), no device assert, no sync.
 * bpm_eval_update: rows [n0, n0 + B) are written (n0 is known to the host from shapes); when `loss` (device pointer to
 * one fp32, the batch's criterion) is given, it is copied to losses[batch_index].
 *
 * bpm_eval_finalize over rows [0, N) and losses [0, nbatches):   result[0] = mean of the batch losses (NaN for none).
 *   BPM_EVAL_MULTILABEL  result (C + 4 doubles): [1 + c] average precision of class c, [1 + C] micro (all N C elements as
 *                        one list), [2 + C] samples (mean over the rows of the row's own list), [3 + C] mean over the rows
 *                        of F1 = 2 |y & p| / (|y| + |p|) (0 when both are empty).
 *                        counts (4 C + 1 int64): [4 c + 0..3] tp, fp, fn, tn of class c; [4 C] rows with every class right.
 *                        AP = (1 / P) sum_{i : y_i = 1} TP>=(s_i) / N>=(s_i), N>=(s) the elements of the list with score
 *                        >= s and TP>=(s) the positives among them: scikit-learn's -sum dR P over distinct thresholds,
 *                        ties included (the k positives tied at a threshold each add that threshold's precision).  A
 *                        list without a positive gives 0.  Cost O(n^2) integer compares per list of n, no sort.
 *   other kinds          result (7 doubles): [1] sum |p - t|, [2] sum p, [3] sum t, [4] sum p p, [5] sum t t, [6] sum p t,
 *                        p = predict (BPM_EVAL_CLASSES: argmax * 6 - 3, exact), t = target.
 *                        counts (8 int64): [0] rintf(p) == rintf(t) (round-half-even, as np.round); over the rows with
 *                        t != 0 the 2 x 2 of p > 0 against t > 0: [1] both, [2] p only, [3] t only, [4] neither;
 *                        [5] argmax == t (BPM_EVAL_CLASSES) / predict == t; [6] rows that take part; [7] rows with t != 0.
 * ws: bpm_eval_ws_bytes(kind, capacity, C) bytes (0 for arguments it does not accept), 8-byte aligned, private to the
 * stream for the call; its contents do not matter before or after.
 * BPM_ERR_ARG (nothing launched): NULL desc or a NULL pointer that the kind uses, B < 1, C < 1 (C != 1 for
 * BPM_EVAL_REGRESSION), capacity < 1, n0 < 0, n0 + B > capacity, ld < C, ldt < C (BPM_EVAL_MULTILABEL), a loss with
 * batch_index outside [0, max_batches), an unknown kind, capacity * C >= 2^31 (BPM_EVAL_MULTILABEL); finalize: N outside
 * [1, capacity], nbatches outside [0, max_batches], NULL result / counts, a workspace that is NULL or too small.
 * BPM_ERR_ALIGN: pointers not 4-byte (int64 targets, result, counts, ws: 8-byte) aligned. */
enum { BPM_EVAL_MULTILABEL = 0, BPM_EVAL_REGRESSION = 1, BPM_EVAL_CLASSES = 2 };
typedef struct bpm_eval_desc {
    int kind;               /* BPM_EVAL_* */
    int C, capacity, max_batches;
    float* score;
    float* predict;
    float* raw;
    float* target;
    unsigned char* pred;
    unsigned char* label;
    float* losses;          /* [max_batches], optional */
    int* bad;               /* optional */
    /* bpm_eval_update */
    const float* logits; int ld;
    const void* targets; int ldt;
    const float* loss;      /* optional */
    int B, n0, batch_index;
    /* bpm_eval_finalize */
    int N, nbatches;
    double* result;
    int64_t* counts;
    void* ws; size_t ws_bytes;
} bpm_eval_desc;
size_t bpm_eval_ws_bytes(int kind, int capacity, int C);
int bpm_eval_update(const bpm_eval_desc* d, void* stream);
int bpm_eval_finalize(const bpm_eval_desc* d, void* stream);

/* Sharded evaluation (data parallelism): every rank evaluates a contiguous share of the batches into its own store;
 * the shards are exchanged as images and merged on the device, in rank order, into every rank's store; the unchanged
 * bpm_eval_finalize then runs everywhere.  Only bit patterns move, so the merged store -- and with it every metric --
 * is bit-identical to an unsharded evaluation over the same batches.  One launch each, no host read.
 *
 * The exchange image: 32-bit words.  For `rows` rows and `batches` losses, with E = rows * C elements
 * (BPM_EVAL_MULTILABEL) or E = rows (other kinds):
 *     [0] bad    [1] void mark    [2, 2 + batches) losses    the 32-bit fields, E words each    the byte fields,
 *     ceil(E / 4) words each, byte i of a field in bits 8 * (i % 4) of its word i / 4.
 *   The void mark is 0 from bpm_eval_pack.  A rank that finds its shard is not what the ranks agreed on leaves its
 *   slot zero and sets this word instead of packing; bpm_eval_merge then writes *bad = -1 (never a count), which the
 *   caller's one host read finds on every rank.
 *   BPM_EVAL_MULTILABEL  score | pred, label        BPM_EVAL_REGRESSION  score, predict, raw, target
 *   BPM_EVAL_CLASSES     predict, target | label
 * bpm_eval_image_bytes(kind, rows, batches, C): the bytes of that image (0 for arguments it does not accept: an unknown
 * kind, rows < 0, batches < 0, C < 1, C != 1 for BPM_EVAL_REGRESSION, rows * C >= 2^31 for BPM_EVAL_MULTILABEL).
 *
 * bpm_eval_pack: rows [0, n), losses [0, nb) and *bad (0 when NULL) of the store in `d` into `image`, laid out for
 * (rows, batches) >= (n, nb) -- ranks exchange images of one common size, that of the largest shard.  Every word of
 * image[0, image_bytes / 4) is written; the words beyond the shard's own data are zero, so the image is a function of
 * the shard alone and a sum of images that are zero outside one slot (an integer all-reduce) reproduces it.
 *
 * bpm_eval_merge: `images` holds W images, image_bytes apart, each laid out for (max rows[r], max batches[r]).  Rank
 * r's rows go to rows [sum rows[:r], ...) of the store in `d`, its losses to losses [sum batches[:r], ...), and *bad
 * (when not NULL) becomes the sum of the images' bad words.  rows / batches are HOST arrays of W ints, read before the
 * call returns; a rank with zero rows and zero batches is legal, and so is a merge of nothing (only *bad is written).
 * The store may be the one the local image was packed from (the images are separate memory: pack first).  The byte
 * fields are written with byte stores: a shard may start at any residue of rows * C mod 4.
 * BPM_ERR_ARG (nothing launched): NULL desc / image(s) / rows / batches or a NULL pointer that the kind uses, an unknown
 * kind, C < 1 (C != 1 for BPM_EVAL_REGRESSION), capacity < 1, a negative count, n > capacity, n > rows, nb > batches,
 * nb > max_batches, losses wanted with NULL losses, W outside [1, BPM_EVAL_MAX_RANKS], sum rows > capacity,
 * sum batches > max_batches, image_bytes not a multiple of 4 or less than bpm_eval_image_bytes says.
 * BPM_ERR_ALIGN: store or image pointers not 4-byte aligned. */
#define BPM_EVAL_MAX_RANKS 64
size_t bpm_eval_image_bytes(int kind, int rows, int batches, int C);
int bpm_eval_pack(const bpm_eval_desc* d, int n, int nb, int rows, int batches, void* image, size_t image_bytes, void* stream);
int bpm_eval_merge(const bpm_eval_desc* d, const void* images, size_t image_bytes, int W, const int* rows, const int* batches,
                   void* stream);

/* Engine plumbing (no reference counterpart): a non-blocking HIP stream at the device's lowest priority
 * (low_priority != 0) or at the default priority.  The host engine puts weight-gradient GEMMs and the
 * key/value-side chain there so that the dispatcher serves the critical-path stream first. */
int bpm_stream_create(int low_priority, void** out_stream);
int bpm_stream_priority_range(int* least, int* greatest);

/* ------------------------------------------------------------------------
 * Launch profiler (measurement aid for bench.py; no reference counterpart).
 * While bit `kind` of the mask is set, every launch of that kernel kind is
 * bracketed by two HIP events ON ITS LAUNCH STREAM and its algorithmic work is
 * tallied (GEMM: 2*M*N*K; attention: 2 FLOPs per visible (query,key) pair per
 * head-dim element per algorithmic product, recomputation not counted).
 * bpm_prof_collect waits for the recorded events, returns the summed
 * per-launch durations (ms), work and launch count of one kind, and clears them.
 * ---------------------------------------------------------------------- */
enum { BPM_PROF_GEMM_NT = 0, BPM_PROF_GEMM_NN = 1, BPM_PROF_GEMM_TN = 2, BPM_PROF_ATTN_FWD = 3,
       BPM_PROF_ATTN_BWD_DQ = 4, BPM_PROF_ATTN_BWD_DKV = 5,
       /* bpm_gemm_grouped launches that the LDS-DMA kernel takes (hidden >= 512 shapes) are tallied apart from the
        * 128 x 64 register-staged kernel's (kinds 0-2), so a kind is one kernel */
       BPM_PROF_GEMM_DMA_NT = 13, BPM_PROF_GEMM_DMA_NN = 14, BPM_PROF_GEMM_DMA_TN = 15 };
int bpm_prof_enable(unsigned kind_mask);
int bpm_prof_collect(int kind, double* total_ms, double* total_work, int* launches);
/* The same, plus the launches' ALGORITHMIC HBM bytes (GEMM: both operands once, the output once, every side operand of
 * the epilogue once -- residual, gate, the previous value for +=; attention: Q, K, V, O (+ dO, dQ, dK, dV) once). */
int bpm_prof_collect2(int kind, double* total_ms, double* total_work, double* total_bytes, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* BPMULT_HIP_H */

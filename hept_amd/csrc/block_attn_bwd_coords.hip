// block_attn_bwd_coords: the backward of block_attn_coords_kernel (HEPT_PREC_MIXED16_DIFF, "mixed16_diff") on the rows that
// forward gathers -- the opt-in 16-bit training tiles of that mode (HEPTAttention.train_tiles = "mixed16").  A 16-bit
// sibling of block_attn_bwd_bf16_kernel in a file of its own, so that every existing kernel stays byte-identical.
//
// Rows: the "mixed16" rows (fp16 q^ (H, N, 64 B); fp16 k^ | bf16 v with its 1.0 column at D (H, N, 128 B)), the caller's f32
// coords (N, C) and sqrt_w (H, C).  Per (table, head, block), the two phases of the bf16 backward (phase Q: a wave owns 32
// queries and walks the key tiles; phase K: a wave owns 32 keys and walks the query tiles), all four tiles resident:
//
//   logit          recomputed as the forward forms it, operation for operation: v_mfma_f32_32x32x16_f16 on the stored fp16
//                  values with every column >= D cleared in both operands, on top of the two feature-only norms formed in
//                  f32 in the forward's order (a query's in two interleaved halves, a key's in four pieces of 8 columns);
//                  then -1/2 sum_c (sqrt_w cq_c - sqrt_w ck_c)^2 in f32 from the two LDS side arrays of scaled coordinates,
//                  ascending c.  Rows at and after raw_size count as coordinates 0 in both roles.  P = exp(min(S, 0)) is
//                  the forward's P bit for bit.
//   padding        queries at and after raw_size (src variant) keep the forward's logit, the key's STORED norm.  Where that
//                  norm is not finite, P = 0 and dS is set to exactly 0 (never 0 x inf).  DECISION: their dS reaches a real
//                  key's coordinate columns as -dS . sqrt_w ck_c with ck_c from the f32 `coords`, not from the stored fp16
//                  value -- the padding query's side-array entry is 0, so the general formula below gives just that; the
//                  stored value is rounded to 11 bits (and saturated beyond the fp16 range), the f32 one is what the key's
//                  own logits use.  The padding rows' own gradients are zeroed by hept_bwd_reduce16.
//   dP, dV         dP = G . V^T and dV = P^T . G on the bf16 MFMA, P and dS rounded to bf16 as the bf16 backward rounds them;
//                  dS = dP o P o [S <= 0].  G enters dP in TWO bf16 pieces (bf16(G) and bf16(G - bf16(G)), a fifth resident
//                  tile), unlike the bf16 backward: dP_ij = dnumer_i . v_j + dden_i cancels where the values of a block
//                  agree with the output, and on tight clusters (the case the mode is for) G rounded to 8 bits is 0.20 of
//                  dq's scale by itself -- against 0.01 for the fp16 rows and 0.05 for bf16 rows (float64 emulation of each
//                  rounding alone, profiles/train_mixed16_diff16.txt).  dV = P^T . G takes bf16(G) alone: nothing cancels.
//   d q^ / d k^    feature columns: dS . K^ - rowsum(dS) q^ (and transposed), the row sum riding through the same product
//                  against a 1.0 in column 30 of K^ (31 of Q^).  DECISION: the stored fp16 values enter at their stored
//                  precision by an EXACT split of each fp16 value into two bf16 pieces (hi = bf16(x), lo = x - hi: at most
//                  3 significant bits, exact) and two bf16 MFMAs per product -- the pieces are formed in registers from the
//                  transposed LDS read of the fp16 tile, so no further tile is resident.  The alternative, dS scaled per
//                  block by a power of two into fp16 and one _f16 MFMA, needs a block-wide maximum of |dS| (a reduction
//                  and a barrier in the middle of both phases) and leaves small dS of the block in the fp16 subnormals; it
//                  was not built.
//                  coordinate columns: sum_j dS_ij (sqrt_w ck_c[j] - sqrt_w cq_c[i]) and its transpose, summed as written in
//                  f32 on the VALU from the side arrays (f32 dS); the two lane halves meet in one __shfl_xor, the sums pass
//                  through an LDS stash and the epilogue stores them where the MFMA result of that column would go.
//                  C = 2, 4, 6 are compile-time; any other C walks the coordinate columns BWDC_COLS = 2 at a time INSIDE the
//                  kernel (one launch, one writer per output dword).  The runtime path is NOT a cheap one: the tile loop of
//                  each phase runs ceil(C / 2) times, and every walk repeats all the MFMAs and the full C-column logit and
//                  starts its accumulators again (the last walk's are stored) -- C = 28 does the matrix work 14 times.  No
//                  shipped model takes it (C = 2, 4, 6); two columns is what its 16 extra logit accumulators leave
//                  without scratch.
//
// Outputs: dq_part (Tl, N, H, 32) and dkv_part (Tl, N, H, 64) of bf16, exactly as hept_block_attn_bwd_bf16 writes them;
// hept_bwd_reduce16 sums them.
//
// LDS: five 16-bit tiles (40 KB at B = 128), five 4-byte records per row (norms, stored norm, indices) and three f32 side
// arrays per row (scaled coordinates of the queries, of the keys, the gradient stash): 109 KB at B = 256, C = 6.  The widest
// rows on the largest blocks (C >= 26, i.e. D <= 4, with B > 224) would need more than the 160 KB of a CU: HEPT_ERR_SHAPE.
// Registers, from the compiler's resource remarks (-Rpass-analysis=kernel-resource-usage), two waves per SIMD asked for:
//   C = 2: 110 - 177 VGPRs    C = 4: 142 - 213    C = 6: 164 - 246    runtime C: 180 - 222;   scratch 0 in all 64 instantiations
//   (profiles/train_mixed16_diff16.txt section 7).
// (The tile walks are rolled and the wave's own operand rows are fetched per tile: unrolled, the scheduler hoisted every
//  tile's LDS reads to the top and the six-column instantiations spilled up to 6 KB per lane.)
#include "common.h"

namespace {

constexpr int BPROW = 64;  // bytes of one 32-column 16-bit tile row
__device__ __forceinline__ int plane_chunk(int row, int c) { return row * BPROW + ((c ^ ((row >> 2) & 3)) << 4); }

// (the operand addressing of block_attn_bwd.hip's 16-bit kernel: lane-dependent bases plus compile-time offsets)
struct PlaneLanes {
    int row[2];  // A-operand 16-B chunk of row li, step s:      + tile * 32 * BPROW
    int tr[2];   // transposed 8-B reads, rows +0..3 / +8..11:   + (tile * 32 + 16 s) * BPROW
};
__device__ __forceinline__ PlaneLanes plane_lanes(int lane) {
    const int li = lane & 31, hh = lane >> 5, l16 = lane & 15, g = lane >> 4;
    PlaneLanes p;
    p.row[0] = plane_chunk(li, hh);
    p.row[1] = plane_chunk(li, 2 + hh);
    const int r = 4 * hh + (l16 >> 2), colb = 32 * (g & 1) + 8 * (l16 & 3);
    p.tr[0] = plane_chunk(r, colb >> 4) + (colb & 15);
    p.tr[1] = plane_chunk(r + 8, colb >> 4) + (colb & 15);
    return p;
}
// B-operand fragment (k = the 16 rows starting at byte offset base, n = column li) by transposing reads
__device__ __forceinline__ u32x4 plane_tr_frag(const char* plane, const PlaneLanes& pl, int base) {
    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(plane + base + pl.tr[0]));
    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(plane + base + pl.tr[1]));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x8 vv = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    return __builtin_bit_cast(u32x4, vv);
}
// element (row 32 w + acc_row(r, hh), column li) of a tile: a lane constant plus a compile-time term
struct ElemLanes {
    int base[2];  // r & 4 == 0 / != 0
};
__device__ __forceinline__ ElemLanes elem_lanes(int w, int lane) {
    const int li = lane & 31, hh = lane >> 5;
    ElemLanes e;
    e.base[0] = (w * 32 + 4 * hh) * BPROW + ((((li >> 3) ^ hh) & 3) << 4) + ((li & 7) << 1);
    e.base[1] = e.base[0] ^ 32;
    return e;
}
__device__ __forceinline__ float plane_elem_f16(const char* plane, const ElemLanes& e, int r) {
    const int off = e.base[(r >> 2) & 1] + ((r & 3) + 8 * (r >> 2)) * BPROW;
    return (float)*reinterpret_cast<const _Float16*>(plane + off);
}
__device__ __forceinline__ u32x4 pack8_bf16(const float* a) {
    return u32x4{hept_pack_bf16(a[0], a[1]), hept_pack_bf16(a[2], a[3]), hept_pack_bf16(a[4], a[5]),
                 hept_pack_bf16(a[6], a[7])};
}

// fp16 pair in a dword -> its contribution to the feature norm; the halves at columns >= D are cleared in place
// (block_attn_coords.hip: the same function, so that the norms are the forward's)
__device__ __forceinline__ float feat_word(unsigned int& w, int col0, int D, float acc) {
    const float lo = hept_f16_lo(w), hi = hept_f16_hi(w);
    const bool f0 = col0 < D, f1 = col0 + 1 < D;
    acc = f0 ? fmaf(lo, lo, acc) : acc;
    acc = f1 ? fmaf(hi, hi, acc) : acc;
    w = (f0 ? (w & 0x0000FFFFu) : 0u) | (f1 ? (w & 0xFFFF0000u) : 0u);
    return acc;
}

// eight fp16 values -> two bf16 pieces each, hi + lo == the value exactly (11 significant bits = 8 + at most 3)
__device__ __forceinline__ void split_f16(const u32x4& f, u32x4& hi, u32x4& lo) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = hept_f16_lo(f[j]), b = hept_f16_hi(f[j]);
        const unsigned int hp = hept_pack_bf16(a, b);
        hi[j] = hp;
        lo[j] = hept_pack_bf16(a - hept_bf16_lo(hp), b - hept_bf16_hi(hp));
    }
}
// z += ds . f with f an fp16 fragment at its stored precision: the small piece first
__device__ __forceinline__ f32x16 mfma_ds_f16(const u32x4& ds, const u32x4& f, f32x16 z) {
    u32x4 hi, lo;
    split_f16(f, hi, lo);
    z = mfma_bf16(ds, lo, z);
    return mfma_bf16(ds, hi, z);
}

// exp_clamped (common.h) for one logit: the same IEEE product, v_exp and clamp, so the same value
__device__ __forceinline__ float exp_clamped1(float x) {
    return __builtin_fminf(__builtin_fmaxf(__builtin_amdgcn_exp2f(x * 1.442695041f), 0.f), 1.f);
}

// floats per row of the LDS side arrays: whole 8- / 16-B pieces for the compile-time counts, C for the runtime path
constexpr int coord_stride(int ct) { return ct == 2 ? 2 : (ct == 4 ? 4 : 8); }
constexpr int BWDC_COLS = 2;   // coordinate columns whose gradient one walk of the tiles accumulates (register indices)

// the scaled coordinates of one row of a side array, columns [c0, c0 + CW)
template <int CT>
__device__ __forceinline__ void side_row(const float* row, int c0, int C, float (&out)[CT > 0 ? CT : BWDC_COLS]) {
    if constexpr (CT == 2) {
        const hept_f32x2 a = *reinterpret_cast<const hept_f32x2*>(row);
        out[0] = a[0]; out[1] = a[1];
    } else if constexpr (CT == 4 || CT == 6) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(row);
        out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
        if constexpr (CT == 6) {
            const hept_f32x2 b = *reinterpret_cast<const hept_f32x2*>(row + 4);
            out[4] = b[0]; out[5] = b[1];
        }
    } else {
#pragma unroll
        for (int c = 0; c < BWDC_COLS; ++c) out[c] = c0 + c < C ? row[c0 + c] : 0.f;
    }
}

#ifndef BWDC_WAVES
#define BWDC_WAVES 2
#endif
template <int NKT, bool FULL, int CT>
__global__ __launch_bounds__(64 * NKT) __attribute__((amdgpu_waves_per_eu(BWDC_WAVES, BWDC_WAVES)))
void block_attn_bwd_coords_kernel(
    const char* __restrict__ qhat, const char* __restrict__ kvhat, const int* __restrict__ qpos,
    const int* __restrict__ kpos, const float* __restrict__ gacc, const float* __restrict__ coords,
    const float* __restrict__ sqrt_w, unsigned int* __restrict__ dq_part, unsigned int* __restrict__ dkv_part, int N,
    int H, int D, int C, int B, int nb, int raw_size) {
    constexpr int NT = 64 * NKT, ROWS = 32 * NKT, PL = ROWS * BPROW;
    constexpr int CW = CT > 0 ? CT : BWDC_COLS;
    const int CS = CT > 0 ? coord_stride(CT) : C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* q_s = smem;              // Q^ rows (fp16), columns >= D cleared, column 31 = 1.0
    char* k_s = smem + PL;         // K^ rows (fp16), columns >= D cleared, column 30 = 1.0
    char* v_s = smem + 2 * PL;     // [v | 1.0 at column D | 0] (bf16)
    char* g_s = smem + 3 * PL;     // upstream rows [d numer | d den | 0]: bf16(G) ...
    char* gl_s = smem + 4 * PL;    // ... and bf16(G - bf16(G)), the second piece of dP = G . V^T
    float* qn_s = reinterpret_cast<float*>(smem + 5 * PL);   // feature-only norms -|q|^2 / 2 (written by phase Q)
    float* kn_s = qn_s + ROWS;
    float* ktail_s = kn_s + ROWS;                            // the keys' stored norms (padding queries)
    int* qidx_s = reinterpret_cast<int*>(ktail_s + ROWS);
    int* kidx_s = qidx_s + ROWS;
    float* qc_s = reinterpret_cast<float*>(kidx_s + ROWS);   // [ROWS][CS] sqrt_w . coords of the queries
    float* kc_s = qc_s + ROWS * CS;                          // ... of the keys
    float* dc_s = kc_s + ROWS * CS;                          // the coordinate columns of the gradient on their way out

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, li = lane & 31;
    const int bid = blockIdx.x;
    // the tables of a block run side by side (t fastest), as in the forward: the gathers of a point's rows meet in the L2
    const int tl_ = (int)gridDim.x / (H * nb);
    const int h = bid % H, rest = bid / H, b = rest / tl_, t = rest % tl_;
    const size_t seg = ((size_t)t * H + h) * N + (size_t)b * B;
    const int* __restrict__ qp = qpos + seg;
    const int* __restrict__ kp = kpos + seg;
    const char* __restrict__ kvbase = kvhat + (size_t)h * N * (2 * BPROW);
    const float* __restrict__ sw = sqrt_w + (size_t)h * C;

    // ---- stage Q^ and G: one item = a 16-B chunk (8 columns) of a gathered row; lane c of a row scales coordinates c, c + 4 ..
    for (int ci = tid; ci < ROWS * 4; ci += NT) {
        const int row = ci >> 2, c = ci & 3;
        const bool ok = FULL || row < B;
        const int src = ok ? qp[row] : 0;
        u32x4 qv = {0u, 0u, 0u, 0u}, gv = {0u, 0u, 0u, 0u}, gl = {0u, 0u, 0u, 0u};
        if (ok) {
            qv = *reinterpret_cast<const u32x4*>(qhat + ((size_t)h * N + src) * BPROW + c * 16);
            const float* grow = gacc + ((size_t)src * H + h) * 32 + c * 8;
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(grow), g1 = *reinterpret_cast<const f32x4*>(grow + 4);
            const float ga[8] = {g0[0], g0[1], g0[2], g0[3], g1[0], g1[1], g1[2], g1[3]};
            split2_bf16(ga, gv, gl);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {   // coordinates (possibly inf) and the stored norm leave the tile
            unsigned int wd = qv[j];
            (void)feat_word(wd, 8 * c + 2 * j, D, 0.f);
            qv[j] = wd;
        }
        if (c == 3) {
            qidx_s[row] = ok ? src : -1;
            qv[3] = ok ? 0x3C000000u : 0u;   // columns (30, 31) = (0, 1.0): column sums of dS ride in dS^T . Q^
        }
        *reinterpret_cast<u32x4*>(q_s + plane_chunk(row, c)) = qv;
        *reinterpret_cast<u32x4*>(g_s + plane_chunk(row, c)) = gv;
        *reinterpret_cast<u32x4*>(gl_s + plane_chunk(row, c)) = gl;
        const bool real = ok && src < raw_size;
        const float* __restrict__ crow = coords + (size_t)src * C;
        for (int cc = c; cc < CS; cc += 4) qc_s[row * CS + cc] = (real && cc < C) ? sw[cc] * crow[cc] : 0.f;
    }
    // ---- stage K^ and V as the forward stages them: the eight pieces of a key are eight consecutive lanes (0 .. 3 its k^
    //      row, 4 .. 7 its v row); the k^ pieces drop their columns >= D and leave their share of the feature norm, which
    //      meets in piece 3's lane (DPP row_shr) in the forward's order; lane c of a key also scales coordinate c
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int ci = it * NT + tid;
        const int key = ci >> 3, c = ci & 7;
        u32x4 val = {0u, 0u, 0u, 0u};
        int src = 0;
        const bool kvalid = FULL || key < B;
        if (kvalid) {
            src = kp[key];
            val = *reinterpret_cast<const u32x4*>(kvbase + (size_t)src * (2 * BPROW) + c * 16);
        }
        float sq = 0.f;
        const unsigned int tail = val[3];   // piece 3: -|k^|^2 / 2 over ALL columns, as the row builder stored it
        if (c < 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned int wd = val[j];
                sq = feat_word(wd, 8 * c + 2 * j, D, sq);
                val[j] = wd;
            }
        }
        const int sqi = __builtin_bit_cast(int, sq);
        const float s1 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, sqi, 0x111, 0xF, 0xF, true));
        const float s2 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, sqi, 0x112, 0xF, 0xF, true));
        const float s3 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, sqi, 0x113, 0xF, 0xF, true));
        if (c < 4) {
            if (c == 3) {
                kn_s[key] = -0.5f * (((s3 + s2) + s1) + sq);
                ktail_s[key] = __uint_as_float(tail);
                kidx_s[key] = kvalid ? src : -1;
                val[3] = kvalid ? 0x00003C00u : 0u;   // columns (30, 31) = (1.0, 0): row sums of dS ride in dS . K^
            }
            *reinterpret_cast<u32x4*>(k_s + plane_chunk(key, c)) = val;
        } else {
            *reinterpret_cast<u32x4*>(v_s + plane_chunk(key, c - 4)) = val;
        }
        const bool kreal = kvalid && src < raw_size;
        const float* __restrict__ kcrow = coords + (size_t)src * C;
        for (int cc = c; cc < CS; cc += 8) kc_s[key * CS + cc] = (kreal && cc < C) ? sw[cc] * kcrow[cc] : 0.f;
    }
    __syncthreads();

    const int own = w * 32 + li;  // the query (phase Q) / key (phase K) of this lane
    const bool padded = raw_size < N;   // uniform: the src variant's padding rows are present
    const PlaneLanes pl = plane_lanes(lane);
    const ElemLanes el = elem_lanes(w, lane);

    // =========================== phase Q: d q^ ===========================
    {
        float qn;
        {   // the forward's feature norm of a query: this lane half's columns in order, then the two halves
            float fn = 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    unsigned int wd = *reinterpret_cast<const unsigned int*>(q_s + w * 32 * BPROW + pl.row[s] + 4 * j);
                    fn = feat_word(wd, 16 * s + 8 * hh + 2 * j, D, fn);
                }
            qn = -0.5f * (fn + __shfl_xor(fn, 32));
            if (hh == 0) qn_s[own] = qn;   // for phase K (behind the barrier between the phases)
        }
        const bool qreal = qidx_s[own] < raw_size;
        f32x16 z;
        for (int c0 = 0; c0 < (CT > 0 ? 1 : C); c0 += BWDC_COLS) {   // (runtime C: BWDC_COLS coordinate columns per walk)
            float qc[CW], dc[CW];
            side_row<CT>(qc_s + own * CS, c0, C, qc);
#pragma unroll
            for (int c = 0; c < CW; ++c) dc[c] = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = 0.f;
#pragma unroll 1   // (a rolled walk: nothing is indexed by the tile but addresses, and unrolled the scheduler hoists every tile's reads to the top and spills)
            for (int kt = 0; kt < NKT; ++kt) {
                if (!FULL && kt * 32 >= B) break;
                // (the wave's own operand rows are fetched again for every tile: held across the walk they cost 16 registers
                //  that the six-column instantiations do not have; the clobber keeps the compiler from hoisting the reads)
                asm volatile("" ::: "memory");
                u32x4 qown[2], gown[2], glown[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    qown[s] = *reinterpret_cast<const u32x4*>(q_s + w * 32 * BPROW + pl.row[s]);
                    gown[s] = *reinterpret_cast<const u32x4*>(g_s + w * 32 * BPROW + pl.row[s]);
                    glown[s] = *reinterpret_cast<const u32x4*>(gl_s + w * 32 * BPROW + pl.row[s]);
                }
                f32x16 x, y;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    x[r] = qn + kn_s[kt * 32 + hept_acc_row(r, hh)];
                    y[r] = 0.f;
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int off = kt * 32 * BPROW + pl.row[s];
                    x = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(k_s + off)),
                                                               __builtin_bit_cast(f16x8, qown[s]), x, 0, 0, 0);   // X^T = K^ . Q^T
                    const u32x4 vt = *reinterpret_cast<const u32x4*>(v_s + off);
                    y = mfma_bf16(vt, glown[s], y);                                                              // Y^T = V . G^T,
                    y = mfma_bf16(vt, gown[s], y);                                                               // G in two pieces
                }
                // ---- the coordinate part, as the forward: -(q^_c - k^_c)^2 / 2 from the f32 products, ascending c; then P, dS and
                //      the coordinate columns of the gradient, one logit at a time (a key's side-array row is read once)
                if constexpr (CT == 0) {
                    float dsq[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) dsq[r] = 0.f;
                    for (int c = 0; c < C; ++c) {
                        const float qcv = qc_s[own * CS + c];
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float dl = qcv - kc_s[(kt * 32 + hept_acc_row(r, hh)) * CS + c];
                            dsq[r] = fmaf(dl, dl, dsq[r]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) x[r] = fmaf(-0.5f, dsq[r], x[r]);
                }
                u32x4 dsb[2];   // dS as bf16 pairs, the A operand of the products below
                float dprev = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kt * 32 + hept_acc_row(r, hh);
                    float kv[CW];
                    side_row<CT>(kc_s + key * CS, c0, C, kv);
                    float xs = x[r];
                    if constexpr (CT > 0) {
                        const float d0 = qc[0] - kv[0];
                        float dsq = d0 * d0;
#pragma unroll
                        for (int c = 1; c < CT; ++c) {
                            const float dl = qc[c] - kv[c];
                            dsq = fmaf(dl, dl, dsq);
                        }
                        xs = fmaf(-0.5f, dsq, xs);
                    }
                    if (padded) xs = qreal ? xs : ktail_s[key];   // padding queries: the key's stored norm, as the forward
                    const float pe = exp_clamped1(xs);
                    // (P = 0: exactly 0, also for a logit of -inf.  The padded slots of a ragged tile need no mask: their V and G
                    //  rows are staged as zeros, 1.0 column included, so dP and with it dS is exactly 0 there)
                    const float d = (xs <= 0.f && pe > 0.f) ? pe * y[r] : 0.f;
#pragma unroll
                    for (int c = 0; c < CW; ++c) dc[c] = fmaf(d, kv[c] - qc[c], dc[c]);
                    if (r & 1) dsb[r >> 3][(r >> 1) & 3] = hept_pack_bf16(dprev, d);
                    dprev = d;
                }
#pragma unroll
                for (int s = 0; s < 2; ++s)   // Z += dS . K^ ; column 30 = rowsum(dS)
                    z = mfma_ds_f16(dsb[s], plane_tr_frag(k_s, pl, (kt * 32 + 16 * s) * BPROW), z);
            }
#pragma unroll
            for (int c = 0; c < CW; ++c) {   // the two halves of the lane pair hold the two halves of the keys
                const float tot = dc[c] + __shfl_xor(dc[c], 32);
                if (hh == 0 && c0 + c < C) dc_s[own * CS + c0 + c] = tot;
            }
        }
        __syncthreads();   // the stash, and qn_s for phase K
        unsigned int* __restrict__ dst = dq_part + (size_t)t * N * H * 16 + (size_t)h * 16 + (li >> 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q2 = w * 32 + hept_acc_row(r, hh);
            const float rs = __shfl(z[r], 30 + 32 * hh);
            const float qv = plane_elem_f16(q_s, el, r);
            float mine = li < D ? z[r] - rs * qv : 0.f;
            if (li >= D && li < D + C) mine = dc_s[q2 * CS + (li - D)];
            const float nbr = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, mine), 0xB1, 0xF,
                                                                                 0xF, true));  // lane ^ 1
            if ((FULL || q2 < B) && (li & 1) == 0) dst[(size_t)qidx_s[q2] * H * 16] = hept_pack_bf16(mine, nbr);
        }
    }

    // =========================== phase K: d k^, d v ===========================
    {
        const float kn = kn_s[own], ktail = ktail_s[own];
        f32x16 zk, zv;
        for (int c0 = 0; c0 < (CT > 0 ? 1 : C); c0 += BWDC_COLS) {
            float kc[CW], dc[CW];
            side_row<CT>(kc_s + own * CS, c0, C, kc);
#pragma unroll
            for (int c = 0; c < CW; ++c) dc[c] = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { zk[r] = 0.f; zv[r] = 0.f; }
#pragma unroll 1
            for (int qt = 0; qt < NKT; ++qt) {
                if (!FULL && qt * 32 >= B) break;
                asm volatile("" ::: "memory");   // (as in phase Q)
                u32x4 kown[2], vown[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    kown[s] = *reinterpret_cast<const u32x4*>(k_s + w * 32 * BPROW + pl.row[s]);
                    vown[s] = *reinterpret_cast<const u32x4*>(v_s + w * 32 * BPROW + pl.row[s]);
                }
                f32x16 x, y;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    x[r] = qn_s[qt * 32 + hept_acc_row(r, hh)] + kn;
                    y[r] = 0.f;
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int off = qt * 32 * BPROW + pl.row[s];
                    x = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(q_s + off)),
                                                               __builtin_bit_cast(f16x8, kown[s]), x, 0, 0, 0);   // X = Q^ . K^T
                    y = mfma_bf16(*reinterpret_cast<const u32x4*>(gl_s + off), vown[s], y);                      // Y = G . V^T,
                    y = mfma_bf16(*reinterpret_cast<const u32x4*>(g_s + off), vown[s], y);                       // G in two pieces
                }
                if constexpr (CT == 0) {
                    float dsq[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) dsq[r] = 0.f;
                    for (int c = 0; c < C; ++c) {
                        const float kcv = kc_s[own * CS + c];
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float dl = qc_s[(qt * 32 + hept_acc_row(r, hh)) * CS + c] - kcv;
                            dsq[r] = fmaf(dl, dl, dsq[r]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) x[r] = fmaf(-0.5f, dsq[r], x[r]);
                }
                u32x4 prb[2], dsb[2];
                float pprev = 0.f, dprev = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qry = qt * 32 + hept_acc_row(r, hh);
                    float qv[CW];
                    side_row<CT>(qc_s + qry * CS, c0, C, qv);
                    float xs = x[r];
                    if constexpr (CT > 0) {
                        const float d0 = qv[0] - kc[0];
                        float dsq = d0 * d0;
#pragma unroll
                        for (int c = 1; c < CT; ++c) {
                            const float dl = qv[c] - kc[c];
                            dsq = fmaf(dl, dl, dsq);
                        }
                        xs = fmaf(-0.5f, dsq, xs);
                    }
                    if (padded) xs = qidx_s[qry] < raw_size ? xs : ktail;
                    const float pe = exp_clamped1(xs);   // (a padded query's G row is zero: its P meets zeros in P^T . G)
                    const float d = (xs <= 0.f && pe > 0.f) ? pe * y[r] : 0.f;
#pragma unroll
                    for (int c = 0; c < CW; ++c) dc[c] = fmaf(d, qv[c] - kc[c], dc[c]);
                    if (r & 1) {
                        prb[r >> 3][(r >> 1) & 3] = hept_pack_bf16(pprev, pe);
                        dsb[r >> 3][(r >> 1) & 3] = hept_pack_bf16(dprev, d);
                    }
                    pprev = pe;
                    dprev = d;
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int base = (qt * 32 + 16 * s) * BPROW;
                    zk = mfma_ds_f16(dsb[s], plane_tr_frag(q_s, pl, base), zk);   // dS^T . Q^ ; column 31 = colsum(dS)
                    zv = mfma_bf16(prb[s], plane_tr_frag(g_s, pl, base), zv);     // P^T . G
                }
            }
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                const float tot = dc[c] + __shfl_xor(dc[c], 32);
                if (hh == 0 && c0 + c < C) dc_s[own * CS + c0 + c] = tot;
            }
        }
        __syncthreads();
        unsigned int* __restrict__ dst = dkv_part + (size_t)t * N * H * 32 + (size_t)h * 32 + (li >> 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k2 = w * 32 + hept_acc_row(r, hh);
            const float cs = __shfl(zk[r], 31 + 32 * hh);
            const float kv = plane_elem_f16(k_s, el, r);
            float dkm = li < D ? zk[r] - cs * kv : 0.f;
            if (li >= D && li < D + C) dkm = dc_s[k2 * CS + (li - D)];
            const float dvm = li < D ? zv[r] : 0.f;
            const float dkn = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, dkm), 0xB1, 0xF,
                                                                                 0xF, true));
            const float dvn = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, dvm), 0xB1, 0xF,
                                                                                 0xF, true));
            if ((FULL || k2 < B) && (li & 1) == 0) {
                unsigned int* row = dst + (size_t)kidx_s[k2] * H * 32;
                row[0] = hept_pack_bf16(dkm, dkn);
                row[16] = hept_pack_bf16(dvm, dvn);
            }
        }
    }
}

// bytes of dynamic LDS of an instantiation (cs: floats per row of a side array)
constexpr size_t bwdc_lds(int nkt, int cs) { return (size_t)5 * 32 * nkt * BPROW + 32 * nkt * 20 + (size_t)3 * 32 * nkt * cs * 4; }
constexpr size_t BWDC_LDS_MAX = 160 * 1024;

template <bool FULL, int CT>
int launch_bwdc(int nkt, dim3 grid, hipStream_t st, const char* qhat, const char* kvhat, const int* qpos, const int* kpos,
                const float* gacc, const float* coords, const float* sqrt_w, unsigned int* dq_part, unsigned int* dkv_part,
                int N, int H, int D, int C, int B, int nb, int raw_size) {
#define HEPT_BWDC_CASE(K)                                                                                              \
    case K: {                                                                                                          \
        const size_t lds = bwdc_lds(K, CT > 0 ? coord_stride(CT) : C);                                                 \
        if (lds > BWDC_LDS_MAX) return HEPT_ERR_SHAPE;                                                                 \
        static LdsRaised raised;   /* (raised to the largest request of the instantiation, once per device) */          \
        if (lds > 65536 && hept_raise_lds(raised, reinterpret_cast<const void*>(&block_attn_bwd_coords_kernel<K, FULL, CT>), \
                                          CT > 0 ? lds : BWDC_LDS_MAX))                                                \
            return HEPT_ERR_LAUNCH;                                                                                    \
        hipLaunchKernelGGL((block_attn_bwd_coords_kernel<K, FULL, CT>), grid, dim3(64 * K), lds, st, qhat, kvhat, qpos, \
                           kpos, gacc, coords, sqrt_w, dq_part, dkv_part, N, H, D, C, B, nb, raw_size);                \
        break;                                                                                                         \
    }
    switch (nkt) {
        HEPT_BWDC_CASE(1)
        HEPT_BWDC_CASE(2)
        HEPT_BWDC_CASE(3)
        HEPT_BWDC_CASE(4)
        HEPT_BWDC_CASE(5)
        HEPT_BWDC_CASE(6)
        HEPT_BWDC_CASE(7)
        HEPT_BWDC_CASE(8)
        default:
            return HEPT_ERR_SHAPE;
    }
#undef HEPT_BWDC_CASE
    return hept_launch_status();
}

}  // namespace

extern "C" int hept_block_attn_bwd_coords(const void* qhat, const void* kvhat, const int32_t* qpos, const int32_t* kpos,
                                          const float* gacc, const float* coords, const float* sqrt_w, int raw_size, int N,
                                          int H, int D, int C, int Tl, int B, void* dq_part16, void* dkv_part16,
                                          void* stream) {
    unsigned int* dq_part = reinterpret_cast<unsigned int*>(dq_part16);
    unsigned int* dkv_part = reinterpret_cast<unsigned int*>(dkv_part16);
    if (!qhat || !kvhat || !qpos || !kpos || !gacc || !coords || !sqrt_w || !dq_part || !dkv_part) return HEPT_ERR_ARG;
    const int rc = hept_check_shape(N, H, D, C, Tl, B);
    if (rc) return rc;
    if (raw_size < 0 || raw_size > N) return HEPT_ERR_SHAPE;
    const int nb = N / B, nkt = (B + 31) / 32;
    const bool full = B == 32 * nkt;
    const dim3 grid((unsigned)((size_t)Tl * nb * H));
    hipStream_t st = (hipStream_t)stream;
    const char* q = reinterpret_cast<const char*>(qhat);
    const char* kv = reinterpret_cast<const char*>(kvhat);
#define HEPT_BWDC_GO(CT)                                                                                                 \
    return full ? launch_bwdc<true, CT>(nkt, grid, st, q, kv, qpos, kpos, gacc, coords, sqrt_w, dq_part, dkv_part, N, H, D, \
                                        C, B, nb, raw_size)                                                              \
                : launch_bwdc<false, CT>(nkt, grid, st, q, kv, qpos, kpos, gacc, coords, sqrt_w, dq_part, dkv_part, N, H, D, \
                                         C, B, nb, raw_size)
    if (C == 2) HEPT_BWDC_GO(2);
    if (C == 4) HEPT_BWDC_GO(4);
    if (C == 6) HEPT_BWDC_GO(6);
    HEPT_BWDC_GO(0);
#undef HEPT_BWDC_GO
}

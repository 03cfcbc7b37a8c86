// block_attn_coords: the 16-bit block attention of block_attn.hip with the COORDINATE part of the logit in f32
// (HEPT_PREC_MIXED16_DIFF, "mixed16_diff").  A sibling of block_attn_kernel<.., BF16, .., F16QK> in a file of its own, so
// that the existing instantiations stay byte-identical and the two files compile side by side.
//
// The rows are the "mixed16" rows (fp16 q^ / k^, bf16 v with the 1.0 column at D).  They round sqrt_w . coords to 11 bits,
// and with the shipped checkpoint's sqrt_w (up to 5.8e3) on raw coordinates that rounding IS the logit error (DESIGN.md
// section 4, case G7); beyond 65504 the stored value is not even finite.  Here, for query i and key j:
//
//   feature part     q.k - |q|^2/2 - |k|^2/2 over the columns d < D of the stored fp16 rows: v_mfma_f32_32x32x16_f16 with
//                    every column from D on CLEARED in both operands (the query's in registers, the keys' while they are
//                    staged -- an fp16 coordinate that overflowed to inf never meets the matrix pipe), both norms formed here
//                    in f32 from the rounded feature values (the norm in the row tail covers the coordinates: not used for a real query)
//   coordinate part  -1/2 sum_c (sqrt_w[h,c] cq_c - sqrt_w[h,c] ck_c)^2 in f32, cq / ck the points' rows of the caller's f32
//                    `coords` (N, C) gathered by qpos / kpos (1.4 MB at 60k points, shared by all heads and tables: it
//                    lives in L2), the difference of the two f32 products as "fp32_diff" forms it.  Rows at and after
//                    raw_size (src variant) count as coordinates 0 in both roles, as the reference's zero rows do.
//   padding queries  (src variant, rows at and after raw_size: zero q^ rows) keep the logit "mixed16" gives them, the key's
//                    stored norm: they carry no point, and the two modes agree on them bit for bit.
//
// The query's scaled coordinates stay in registers (C = 2, 4, 6: compile-time; any other C: recomputed per key tile from the
// L1-resident row), the keys' go to an LDS side array beside k_s / v_s (a broadcast read: one key per lane half).
// Everything after the logit is the 16-bit kernel: clamp at 0, exp, P to bf16, V through the transposed LDS reads, f32
// accumulation, the denominator from the 1.0 column, packed 64-B partial rows at D = 24 and f32 rows otherwise.
// No one-sided push workgroups and no direct scatter: table sharding does not run this mode.
#include "common.h"

namespace {

__device__ __forceinline__ void store16_rows_nt(unsigned int* dst, const u32x4& v) {   // see block_attn.hip: store16_rows
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(dst));
}

// fp16 pair in a dword -> its contribution to the feature norm; the halves at columns >= D are cleared in place
__device__ __forceinline__ float feat_word(unsigned int& w, int col0, int D, float acc) {
    const float lo = hept_f16_lo(w), hi = hept_f16_hi(w);
    const bool f0 = col0 < D, f1 = col0 + 1 < D;
    acc = f0 ? fmaf(lo, lo, acc) : acc;
    acc = f1 ? fmaf(hi, hi, acc) : acc;
    w = (f0 ? (w & 0x0000FFFFu) : 0u) | (f1 ? (w & 0xFFFF0000u) : 0u);
    return acc;
}

// floats per key of the LDS side array: whole 8- / 16-B pieces for the compile-time counts, C for the runtime path
constexpr int coord_stride(int ct) { return ct == 2 ? 2 : (ct == 4 ? 4 : 8); }

// Register budget (an accuracy mode: fewer than the 8 waves per SIMD of the plain 16-bit kernel), from the compiler's
// resource remarks: C = 2, 4, 6 need up to 80 VGPRs on full tiles (6 waves) and 94 on ragged ones (5 waves); the runtime-C
// path keeps 16 more accumulators and spilled 52-160 B per lane at 5 waves: 4 waves = up to 122 VGPRs.  No scratch in any
// instantiation.
constexpr int coords_waves(int ct, bool full) { return ct == 0 ? 4 : (full ? 6 : 5); }

template <int NKT, bool P16, bool FULL, int CT>
__global__ __launch_bounds__(64 * NKT) __attribute__((amdgpu_waves_per_eu(coords_waves(CT, FULL), coords_waves(CT, FULL))))
void block_attn_coords_kernel(const char* __restrict__ qhat, const char* __restrict__ kvhat,
                              const int* __restrict__ qpos, const int* __restrict__ kpos,
                              const float* __restrict__ coords, const float* __restrict__ sqrt_w,
                              float* __restrict__ part, int N, int H, int D, int C, int B, int nb, int raw_size,
                              HeadRange hr) {
    constexpr int NT = 64 * NKT;
    constexpr int KEYS = 32 * NKT;
    constexpr int QROW = 64;          // bytes of a q^ (or k^, or v) row
    constexpr int KVROW = 2 * QROW;   // k^ row | v row
    constexpr int CH = 4, CPR = 8;    // 16-B chunks per k^ (or v) row, per kvhat row
    const int CS = CT > 0 ? coord_stride(CT) : C;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* k_s = smem;
    char* v_s = smem + KEYS * QROW;
    float* kn_s = reinterpret_cast<float*>(smem + 2 * KEYS * QROW);
    int* qidx_s = reinterpret_cast<int*>(smem + 2 * KEYS * QROW + KEYS * 4);
    float* ktail_s = reinterpret_cast<float*>(smem + 2 * KEYS * QROW + KEYS * 8);   // the keys' stored norms (padding queries)
    float* kc_s = reinterpret_cast<float*>(smem + 2 * KEYS * QROW + KEYS * 12);     // [KEYS][CS] sqrt_w . coords of the keys

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, li = lane & 31;
    const int bid = (int)blockIdx.x;
    const int h = hr.h0 + bid % hr.hg;
    const int rest = bid / hr.hg;
    const int b = hr.tl > 0 ? rest / hr.tl : rest % nb, t = hr.tl > 0 ? rest % hr.tl : rest / nb;
    const size_t seg = ((size_t)t * H + h) * N + (size_t)b * B;
    const int* __restrict__ kp = kpos + seg;
    const int* __restrict__ qp = qpos + seg;
    const char* __restrict__ qbase = qhat + (size_t)h * N * QROW;
    const char* __restrict__ kvbase = kvhat + (size_t)h * N * KVROW;
    const float* __restrict__ sw = sqrt_w + (size_t)h * C;

    // ---- this wave's 32 query rows: HBM -> registers (B-operand layout: step s, lane half hh = columns 16 s + 8 hh .. + 7)
    const int qi = w * 32 + li;
    const bool qvalid = FULL || qi < B;
    const int qsrc = qp[qvalid ? qi : 0];
    if (hh == 0) qidx_s[qi] = qvalid ? qsrc : -1;
    const char* qrow = qbase + (size_t)qsrc * QROW;
    u32x4 qraw[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) qraw[s] = *reinterpret_cast<const u32x4*>(qrow + s * 32 + hh * 16);
    float qn;
    {
        float fn = 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned int wd = qraw[s][j];
                fn = feat_word(wd, 16 * s + 8 * hh + 2 * j, D, fn);
                qraw[s][j] = wd;
            }
        qn = -0.5f * (fn + __shfl_xor(fn, 32));
    }
    const bool qreal = qsrc < raw_size;
    const float* __restrict__ qcrow = coords + (size_t)qsrc * C;
    float qc[CT > 0 ? CT : 1];
    if constexpr (CT > 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c) qc[c] = qreal ? sw[c] * qcrow[c] : 0.f;
    }

    // ---- stage K^ and V tiles: gathered rows, 16 B per lane (the eight pieces of a key are eight consecutive lanes:
    //      0 .. 3 its k^ row, 4 .. 7 its v row), K^ XOR-swizzled.  The k^ pieces drop their columns >= D and leave their
    //      share of the feature norm, which meets in piece 3's lane (DPP row_shr); lane c of a key also scales coordinate c
#pragma unroll
    for (int it = 0; it < CPR / 2; ++it) {
        const int ci = it * NT + tid;
        const int key = ci / CPR, c = ci % CPR;
        u32x4 val = {0u, 0u, 0u, 0u};
        int src = 0;
        const bool kvalid = FULL || key < B;
        if (kvalid) {
            src = kp[key];
            val = *reinterpret_cast<const u32x4*>(kvbase + (size_t)src * KVROW + c * 16);
        }
        float sq = 0.f;
        const unsigned int tail = val[3];   // piece 3: -|k^|^2 / 2 over ALL columns, as the row builder stored it
        if (c < CH) {
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
        if (c < CH) {
            if (c == CH - 1) {
                kn_s[key] = -0.5f * (((s3 + s2) + s1) + sq);
                ktail_s[key] = __uint_as_float(tail);
            }
            *reinterpret_cast<u32x4*>(k_s + key * QROW + ((c ^ ((key >> 2) & 3)) * 16)) = val;
        } else {
            *reinterpret_cast<u32x4*>(v_s + key * QROW + (c - CH) * 16) = val;
        }
        const bool kreal = kvalid && src < raw_size;
        const float* __restrict__ kcrow = coords + (size_t)src * C;
        if constexpr (CT > 0) {
            if (c < coord_stride(CT)) kc_s[key * coord_stride(CT) + c] = (kreal && c < CT) ? sw[c] * kcrow[c] : 0.f;
        } else {
            for (int cc = c; cc < C; cc += CPR) kc_s[key * CS + cc] = kreal ? sw[cc] * kcrow[cc] : 0.f;
        }
    }
    __syncthreads();

    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;

#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
        if (!FULL && kt * 32 >= B) break;  // uniform
        const int key = kt * 32 + li;
        f32x16 x;
#pragma unroll
        for (int r = 0; r < 16; ++r) x[r] = qn + kn_s[kt * 32 + hept_acc_row(r, hh)];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int c = 2 * s + hh;
            const u32x4 kraw = *reinterpret_cast<const u32x4*>(k_s + key * QROW + ((c ^ ((key >> 2) & 3)) * 16));
            x = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, kraw), __builtin_bit_cast(f16x8, qraw[s]),
                                                       x, 0, 0, 0);
        }

        // ---- the coordinate part: -(q^_c - k^_c)^2 / 2 from the f32 products, summed in ascending c
        if constexpr (CT > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* kc = kc_s + (kt * 32 + hept_acc_row(r, hh)) * coord_stride(CT);   // (a broadcast: one key per lane half)
                float kv[CT];
                if constexpr (CT == 2) {
                    const hept_f32x2 k0 = *reinterpret_cast<const hept_f32x2*>(kc);
                    kv[0] = k0[0]; kv[1] = k0[1];
                } else {
                    const f32x4 k0 = *reinterpret_cast<const f32x4*>(kc);
                    kv[0] = k0[0]; kv[1] = k0[1]; kv[2] = k0[2]; kv[3] = k0[3];
                    if constexpr (CT == 6) {
                        const hept_f32x2 k1 = *reinterpret_cast<const hept_f32x2*>(kc + 4);
                        kv[4] = k1[0]; kv[5] = k1[1];
                    }
                }
                const float d0 = qc[0] - kv[0];
                float dsq = d0 * d0;
#pragma unroll
                for (int c = 1; c < CT; ++c) {
                    const float dl = qc[c] - kv[c];
                    dsq = fmaf(dl, dl, dsq);
                }
                x[r] = fmaf(-0.5f, dsq, x[r]);
            }
        } else {
            float dsq[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) dsq[r] = 0.f;
            for (int c = 0; c < C; ++c) {
                const float qcv = qreal ? sw[c] * qcrow[c] : 0.f;   // (the query's row: an L1 hit)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float dl = qcv - kc_s[(kt * 32 + hept_acc_row(r, hh)) * CS + c];
                    dsq[r] = fmaf(dl, dl, dsq[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) x[r] = fmaf(-0.5f, dsq[r], x[r]);
        }

        // ---- the src variant's padding queries (rows at and after raw_size: a zero q^ row, stored norm included): their logit is
        //      what "mixed16" forms for them, q^.k^ - |q^|^2/2 - |k^|^2/2 = the key's STORED norm, so that those rows -- which
        //      carry no point, only the block's residual path -- come out of both modes bit for bit the same
        if (raw_size < N) {   // uniform
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float stored = ktail_s[kt * 32 + hept_acc_row(r, hh)];
                x[r] = qreal ? x[r] : stored;
            }
        }

        float pr[16];
        exp_clamped(x, pr);
        if (!FULL && (kt + 1) * 32 > B) {  // ragged last tile: padded keys carry no weight
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt * 32 + hept_acc_row(r, hh) >= B) pr[r] = 0.f;
        }

        const int g = lane >> 4, l16 = lane & 15;
        const int vrow = kt * 32 + 4 * hh + (l16 >> 2);
        const int vcol = 32 * (g & 1) + 8 * (l16 & 3);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u32x4 pw;
#pragma unroll
            for (int j = 0; j < 4; ++j) pw[j] = hept_pack_bf16(pr[8 * s + 2 * j], pr[8 * s + 2 * j + 1]);
            const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(v_s + (vrow + 16 * s) * QROW + vcol));
            const s16x4 v1 =
                __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(v_s + (vrow + 16 * s + 8) * QROW + vcol));
            typedef __attribute__((ext_vector_type(8))) short s16x8;
            const s16x8 vv = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
            z = mfma_bf16(pw, __builtin_bit_cast(u32x4, vv), z);
        }
    }

    if constexpr (P16) {
        // ---- scatter, 64-B rows [24 bf16 numer | f32 denom | 0]: as block_attn_kernel (the tile passes through the dead
        //      K^ / V tiles, a lane stores a 16-B piece)
        __syncthreads();   // every wave is done reading k_s / v_s
        float* tile = reinterpret_cast<float*>(smem) + w * 32 * 32;
        {
            float* wr = tile + (4 * hh) * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) wr[((r & 3) + 8 * (r >> 2)) * 32] = z[r];
        }
        unsigned int* __restrict__ pt =
            reinterpret_cast<unsigned int*>(part) + (size_t)t * hr.tstride_rows * 16 + (size_t)(h - hr.hsub) * 16;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = (lane >> 2) + 16 * j, pc = lane & 3;
            const int q2 = w * 32 + row;
            const f32x4 f0 = *reinterpret_cast<const f32x4*>(tile + row * 32 + pc * 8);
            const f32x4 f1 = *reinterpret_cast<const f32x4*>(tile + row * 32 + pc * 8 + 4);
            u32x4 v = {hept_pack_bf16(f0[0], f0[1]), hept_pack_bf16(f0[2], f0[3]), hept_pack_bf16(f1[0], f1[1]),
                       hept_pack_bf16(f1[2], f1[3])};
            if (pc == 3) v = u32x4{__float_as_uint(f0[0] + 1e-20f), 0u, 0u, 0u};   // example/hept.py:14
            if (FULL || q2 < B) store16_rows_nt(pt + (size_t)qidx_s[q2] * hr.hout * 16 + pc * 4, v);
        }
    } else {
        // ---- scatter: row = 32 floats = one 128-B line per query, lanes 0..31 contiguous
        float* __restrict__ pt = part + (size_t)t * hr.tstride_rows * 32 + (size_t)(h - hr.hsub) * 32 + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q2 = w * 32 + hept_acc_row(r, hh);
            if (FULL || q2 < B) {
                float val = z[r];
                if (li == D) val += 1e-20f;  // example/hept.py:14
                pt[(size_t)qidx_s[q2] * hr.hout * 32] = val;
            }
        }
    }
}

template <bool P16, bool FULL, int CT>
int launch_coords(int nkt, dim3 grid, hipStream_t st, const char* qhat, const char* kvhat, const int* qpos, const int* kpos,
                  const float* coords, const float* sqrt_w, float* part, int N, int H, int D, int C, int B, int nb,
                  int raw_size, HeadRange hr) {
#define HEPT_COORDS_CASE(K)                                                                                          \
    case K: {                                                                                                        \
        const size_t lds = (size_t)2 * 32 * K * 64 + 32 * K * 12 + (size_t)32 * K * 4 * (CT > 0 ? coord_stride(CT) : C); \
        hipLaunchKernelGGL((block_attn_coords_kernel<K, P16, FULL, CT>), grid, dim3(64 * K), lds, st, qhat, kvhat, qpos,  \
                           kpos, coords, sqrt_w, part, N, H, D, C, B, nb, raw_size, hr);                                 \
        break;                                                                                                       \
    }
    switch (nkt) {
        HEPT_COORDS_CASE(1)
        HEPT_COORDS_CASE(2)
        HEPT_COORDS_CASE(3)
        HEPT_COORDS_CASE(4)
        HEPT_COORDS_CASE(5)
        HEPT_COORDS_CASE(6)
        HEPT_COORDS_CASE(7)
        HEPT_COORDS_CASE(8)
        default:
            return HEPT_ERR_SHAPE;
    }
#undef HEPT_COORDS_CASE
    return hept_launch_status();
}

template <bool P16, int CT>
int launch_coords_tile(bool full, int nkt, dim3 grid, hipStream_t st, const char* qhat, const char* kvhat, const int* qpos,
                       const int* kpos, const float* coords, const float* sqrt_w, float* part, int N, int H, int D, int C,
                       int B, int nb, int raw_size, HeadRange hr) {
    if (full)
        return launch_coords<P16, true, CT>(nkt, grid, st, qhat, kvhat, qpos, kpos, coords, sqrt_w, part, N, H, D, C, B, nb,
                                            raw_size, hr);
    return launch_coords<P16, false, CT>(nkt, grid, st, qhat, kvhat, qpos, kpos, coords, sqrt_w, part, N, H, D, C, B, nb,
                                         raw_size, hr);
}

}  // namespace

// internal (common.h): the launch behind HEPT_PREC_MIXED16_DIFF; sizes and pointers are checked by block_attn_impl.
// Packed rows (D = 24, every shipped model): C = 2, 4, 6 specialised; any other (D, C): the runtime-C path (C <= 28: at most
// 62 KB of LDS at B = 256).
int hept_block_attn_coords_launch(const void* qhat, const void* kvhat, const int32_t* qpos, const int32_t* kpos,
                                  const float* coords, const float* sqrt_w, int raw_size, int N, int H, int D, int C, int Tl,
                                  int B, const HeadRange& hr, float* part, void* stream) {
    const int nb = N / B, nkt = (B + 31) / 32;
    const bool full = B == 32 * nkt;
    const dim3 grid((unsigned)((size_t)Tl * nb * hr.hg));
    hipStream_t st = (hipStream_t)stream;
    const char* qh = (const char*)qhat;
    const char* kv = (const char*)kvhat;
#define HEPT_COORDS_GO(P16, CT) \
    return launch_coords_tile<P16, CT>(full, nkt, grid, st, qh, kv, qpos, kpos, coords, sqrt_w, part, N, H, D, C, B, nb, raw_size, hr)
    if (D == 24) {
        if (C == 2) HEPT_COORDS_GO(true, 2);
        if (C == 4) HEPT_COORDS_GO(true, 4);
        if (C == 6) HEPT_COORDS_GO(true, 6);
        HEPT_COORDS_GO(true, 0);
    }
    HEPT_COORDS_GO(false, 0);
#undef HEPT_COORDS_GO
}

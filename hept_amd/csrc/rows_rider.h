// riders: the v half of the kvhat rows, written by workgroups that travel in the bucket-sort launch (sort_tables.hip: KB).
// Row-format code (kvhat pitch, the v half's offset, column D); included by sort_tables.hip only.
//
// KB is a chain of short dependent steps per workgroup: it moves 35 MB in 21 us and leaves the memory system idle most
// of that time.  The v role of the row builder (prep_hash.hip: [v | 1.0 at column D | 0 ..] per (head, point)) is the
// opposite -- a pure format conversion of 77 MB with no dependence on anything the forward computes -- so the first
// `vy` rows of the KB grid do it instead of sorting: no LDS and no more registers than KB itself (the launch's
// resources stay KB's).  Same values as the v role (the same bf16 conversion).  Measured at tracking-60k (bf16 / f32
// tiles): row builder 55.2 -> 46.2 / 65.2 -> 53.2 us, sort 37.2 -> 44.3 / 38.0 -> 47.7 us, forward -2.3 us; the riders
// alone take ~20 us (a rider wave is its own chain of load -> convert -> store trips), so more of them (8 grid rows:
// +4 us) or fewer (2: +1 us) are both worse than 3, and the q / k roles that stay behind run at 3.9 TB/s instead of
// the three roles' 4.7 -- the v role was already filling their gaps.
#pragma once
#include <stdlib.h>
#include "common.h"

namespace {   // (one translation unit: the kernels that take a RowsJob live in sort_tables.hip's unnamed namespace too)

struct RowsJob {
    const void* v;      // (N, H * D) fp32, or bf16 / fp16 at an 8-byte aligned base (`in`)
    char* kvhat;        // (H, N, 2 * qrow bytes): v half at byte qrow of a row
    int N, raw_size;    // rows >= raw_size are padding: v = 0 (src variant)
    int H, D4;          // D / 4
    int f32;            // 1: f32 tile rows (qrow = 128 B), 0: 16-bit rows (qrow = 64 B)
    int vy;             // grid rows (of gridDim.x workgroups each) that are riders; 0: none
    int in;             // HEPT_IN_*: element type of v
};
#ifndef HEPT_ROWS_RIDERS
#define HEPT_ROWS_RIDERS 3
#endif

// The type-dependent parts of a rider: a quad (4 consecutive elements of v, one load), the 1.0 of
// column D, and the conversion at the store.  16-bit v (HEPT_IN_BF16 / HEPT_IN_F16): a source address is only 8-byte
// aligned in general (any D % 4 == 0), so a quad is one 8-byte load (half the load registers of the f32 input), widened
// at the store (common.h: hept_widen4); the 1.0 of column D travels as the input type's own 1.0.  bf16 input into bf16
// rows is a repack of the same bits (= hept_pack_bf16 of the widened values: bf16 -> f32 -> bf16 is the identity).
template <int IN>
struct RiderIn {
    typedef unsigned short Elem;
    typedef u32x2 Quad;
    static constexpr unsigned int ONE = IN == HEPT_IN_BF16 ? 0x3F80u : 0x3C00u;   // 1.0 in the low half of a dword
    static __device__ __forceinline__ Quad zero() { return Quad{0u, 0u}; }
    static __device__ __forceinline__ f32x4 f32_piece(const Quad& a) { return hept_widen4<IN>(a[0], a[1]); }
    static __device__ __forceinline__ u32x4 bf16_piece(const Quad& a, const Quad& b) {
        u32x4 out = u32x4{a[0], a[1], b[0], b[1]};
        if constexpr (IN != HEPT_IN_BF16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = hept_pack_bf16(hept_in_lo<IN>(out[j]), hept_in_hi<IN>(out[j]));
        }
        return out;
    }
};
template <>
struct RiderIn<HEPT_IN_F32> {
    typedef float Elem;
    typedef f32x4 Quad;
    static constexpr float ONE = 1.f;
    static __device__ __forceinline__ Quad zero() { return Quad{0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ f32x4 f32_piece(const Quad& a) { return a; }
    static __device__ __forceinline__ u32x4 bf16_piece(const Quad& a, const Quad& b) {
        return u32x4{hept_pack_bf16(a[0], a[1]), hept_pack_bf16(a[2], a[3]), hept_pack_bf16(b[0], b[1]), hept_pack_bf16(b[2], b[3])};
    }
};

// A wave takes a tile of 8 consecutive points (one contiguous run of v) at a time.  A row half is PPR 16-B pieces
// (4 of 8 bf16 values = two quads, or 8 of 4 floats = one quad); lane order inside the tile is [head][point][piece]: a
// store instruction writes whole 64-B / 128-B row halves of consecutive points of one head -- the pattern of the row
// builder's copy-out -- and piece k of row (h, n) reads v[n][h*D + 8k ..] (bf16) or [.. + 4k ..] (f32): elements below
// D are data, element D is the 1.0 that makes P.V produce the denominator (D % 4 == 0: the first element of a quad,
// which is then not loaded), the rest zeros.  All loads of a trip are in flight before the first conversion (trips of
// IT = 2 / 4 instructions, 16 at H = 8 per f32 tile: 4 trips; the riders must not raise the launch's register count
// above KB's own); the 128-B lines of the run are shared by the wave's instructions through L1.
template <int H_, int IN, bool F32, int WAVES>   // H_ == 0: run-time head count; F32: f32 tile rows; WAVES per workgroup
__device__ __forceinline__ void rows_rider_tiles(const RowsJob& jb, unsigned int wg, unsigned int n_wgs) {
    typedef RiderIn<IN> In;
    constexpr unsigned int QUADS = F32 ? 1 : 2, PPR = F32 ? 8 : 4, IT = F32 ? 4 : 2, ROW = F32 ? 256 : 128;
    constexpr bool NT = F32 ? HEPT_NT_RIDER_IN32 : HEPT_NT_RIDER_IN16;
    const unsigned int H = H_ ? H_ : (unsigned int)jb.H, D = 4u * (unsigned int)jb.D4, HD = H * D;
    const unsigned int lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned int ntiles = ((unsigned int)jb.N + 7u) >> 3;
    const unsigned int wave = wg * WAVES + wv, n_waves = n_wgs * WAVES;
    const typename In::Elem* v = reinterpret_cast<const typename In::Elem*>(jb.v);
    for (unsigned int tile = wave; tile < ntiles; tile += n_waves) {
        const unsigned int n0 = tile << 3;
        for (unsigned int i0 = 0; i0 < H * 8 * PPR; i0 += 64 * IT) {
            typename In::Quad x[IT][QUADS];
            unsigned int hd[IT], n[IT], k[IT];
#pragma unroll
            for (unsigned int u = 0; u < IT; ++u) {
                const unsigned int i = i0 + u * 64 + lane;
                k[u] = i & (PPR - 1);
                n[u] = n0 + ((i / PPR) & 7u);
                hd[u] = i / (8 * PPR);
                const bool row = hd[u] < H && n[u] < (unsigned int)jb.raw_size;
                const typename In::Elem* src = v + (size_t)n[u] * HD + hd[u] * D + 4 * QUADS * k[u];
#pragma unroll
                for (unsigned int q = 0; q < QUADS; ++q) {
                    const unsigned int col = 4 * (QUADS * k[u] + q);   // first column of the quad
                    // the 1.0 of column D: f32 rows select it into the piece that is not loaded, 16-bit rows set it after the
                    // two loads (with one form for both the bucket kernel's registers leave 65 / 52: see bucket_body)
                    typename In::Quad fill = In::zero();
                    if constexpr (F32) fill[0] = col == D ? In::ONE : fill[0];
                    x[u][q] = (row && col < D) ? hept_ld<NT>(reinterpret_cast<const typename In::Quad*>(src + 4 * q)) : fill;
                    if constexpr (!F32) { if (col == D) x[u][q][0] = In::ONE; }
                }
            }
#pragma unroll
            for (unsigned int u = 0; u < IT; ++u)
                if (hd[u] < H && n[u] < (unsigned int)jb.N) {
                    char* dst = jb.kvhat + ((size_t)hd[u] * jb.N + n[u]) * ROW + ROW / 2 + k[u] * 16;
                    if constexpr (F32) *reinterpret_cast<f32x4*>(dst) = In::f32_piece(x[u][0]);
                    else *reinterpret_cast<u32x4*>(dst) = In::bf16_piece(x[u][0], x[u][1]);
                }
        }
    }
}

template <int H_, int IN, int WAVES>
__device__ __forceinline__ void rows_rider_in(const RowsJob& jb, unsigned int wg, unsigned int n_wgs) {
    if (jb.f32) rows_rider_tiles<H_, IN, true, WAVES>(jb, wg, n_wgs);
    else rows_rider_tiles<H_, IN, false, WAVES>(jb, wg, n_wgs);
}
template <int H_, int WAVES>
__device__ __forceinline__ void rows_rider(const RowsJob& jb, unsigned int wg, unsigned int n_wgs) {
    if (jb.in == HEPT_IN_BF16) return rows_rider_in<H_, HEPT_IN_BF16, WAVES>(jb, wg, n_wgs);
    if (jb.in == HEPT_IN_F16) return rows_rider_in<H_, HEPT_IN_F16, WAVES>(jb, wg, n_wgs);
    rows_rider_in<H_, HEPT_IN_F32, WAVES>(jb, wg, n_wgs);
}

// the job of the rider workgroups, from the description a caller in another translation unit hands over
RowsJob rows_job(const HeptRowsJob* r) {
    RowsJob jb{};
    if (!r) return jb;
    jb.v = r->v;
    jb.kvhat = reinterpret_cast<char*>(r->kvhat);
    jb.N = r->N;
    jb.raw_size = r->raw_size;
    jb.H = r->H;
    jb.D4 = r->D / 4;
    jb.f32 = hept_f32_rows(r->precision) ? 1 : 0;
    static const char* const env = getenv("HEPT_ROW_RIDERS");   // (HEPT_ROW_RIDERS=<grid rows>: tuning; read once)
    static const int env_rows = env ? atoi(env) : 0;
    jb.vy = env_rows > 0 && env_rows <= 64 ? env_rows : HEPT_ROWS_RIDERS;
    jb.in = r->in_dtype;
    return jb;
}

}  // namespace

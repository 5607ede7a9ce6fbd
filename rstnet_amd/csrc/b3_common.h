// Three-plane bf16 arithmetic shared by the kernels that run fp32 contractions on the bf16 matrix instruction (gemm_win.hip,
// resblock_b3.hip): an fp32 number is EXACTLY hi + mid + lo with hi = rne_bf16(x), mid = rne_bf16(x - hi), lo = rne_bf16(x - hi - mid)
// (8 + 8 + 8 significand bits; both subtractions are exact in fp32), so an fp32 product is the sum of nine bf16 products, each exact in
// the matrix core's fp32 accumulator.  Six are kept -- lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi, added smallest first -- and the
// three dropped (mid*lo, lo*mid, lo*lo) are below 2^-23 |x||w|, one fp32 rounding of the product.
#pragma once
#include "rst_common.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// two fp32 -> the two packed bf16 (round to nearest even) and the exact remainders
__device__ __forceinline__ unsigned b3_peel(f32x2& v) {
    const unsigned h = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
    v[0] -= __uint_as_float(h << 16);
    v[1] -= __uint_as_float(h & 0xffff0000u);
    return h;
}

// the fp32 values of a staged row piece as two pairs, ready to peel: padding cleared (MK: mask is all ones for data, zero for padding),
// ELU applied
template <bool MK, bool ELU>
__device__ __forceinline__ void b3_take_a(const f32x4 src, const int mask, f32x2 (&v)[2]) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    f32x4 x = src;
    if (MK) x = __builtin_bit_cast(f32x4, __builtin_bit_cast(i32x4, x) & mask);
    if (ELU) {
        x[0] = rst_elu(x[0]); x[1] = rst_elu(x[1]); x[2] = rst_elu(x[2]); x[3] = rst_elu(x[3]);
    }
    v[0] = f32x2{x[0], x[1]};
    v[1] = f32x2{x[2], x[3]};
}

// the accumulators of a wave's TM x TN blocks of 32 x 32, at the start of a tile
template <int TM, int TN>
__device__ __forceinline__ void b3_clear(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
}

// ---- window-sharing tiles of the conv GEMMs (gemm_win_b3_stream_shared_kernel) --------------------------------------------------------
// A causal convolution whose window is R groups of G = S * C floats (K = R * G, left padding (R - 1) * S frames) reads, for output
// row t of an utterance, the groups t - (R - 1) .. t of that utterance's flat activations.  A row tile stages 128 consecutive groups
// ("slab rows") ONCE and multiplies them R times, shifted by one row per tap: slab row r of the tile that starts at output row t0 is
// group t0 + r - (R - 1), accumulator row i (output row t0 + i) sums slab rows i .. i + R - 1, and the last R - 1 accumulator rows of a
// tile have no complete window -- tiles are therefore placed 128 - (R - 1) output rows apart and never cross an utterance.
// Everything a tile's addresses and stores depend on is computed here, for the kernel and for the host-side test that enumerates it.
constexpr int B3_SH_ROWS = 128;               // slab rows per tile

struct B3SharedTile {
    int b, t0;                       // utterance, first output row of the tile inside it
    long m0, mlim;                   // global output rows [m0, mlim) are stored by this tile (m0 = b * T_out + t0)
};
struct B3SharedRow {
    unsigned ao;                     // byte offset from the activations' base of k-tile 0 of the row's group (+ the thread's 16 bytes)
    int klo, kn;                     // k-tiles klo .. klo + kn - 1 of the group lie inside the utterance (klo is always 0 here)
};

__host__ __device__ __forceinline__ constexpr int b3_shared_step(int R) { return B3_SH_ROWS - (R - 1); }
__host__ __device__ __forceinline__ constexpr int b3_shared_tiles_per_utt(int T_out, int R) { return (T_out + b3_shared_step(R) - 1) / b3_shared_step(R); }

__host__ __device__ __forceinline__ B3SharedTile b3_shared_tile(int mt, int R, int T_out) {
    const int tpu = b3_shared_tiles_per_utt(T_out, R), step = b3_shared_step(R);
    B3SharedTile t;
    t.b = mt / tpu;
    t.t0 = (mt - t.b * tpu) * step;
    t.m0 = (long)t.b * T_out + t.t0;
    t.mlim = (long)t.b * T_out + (t.t0 + step < T_out ? t.t0 + step : T_out);
    return t;
}

// slab row r (0 .. 127) of a tile; lk: the thread's first float inside a 16-float k-tile (0, 4, 8, 12); G = S * C floats per group
// (a multiple of 16), TC = T_in * C floats per utterance.  Groups in front of / behind the utterance are all padding: kn = 0 and the
// loads are parked on the first bytes of x; a group the utterance ends in keeps the k-tiles in front of the end.
__host__ __device__ __forceinline__ B3SharedRow b3_shared_row(const B3SharedTile& t, int r, int R, int G, int TC, long x_bstride, int lk) {
    const long g = (long)t.t0 + r - (R - 1);
    const long f0 = g * G;
    B3SharedRow o;
    o.klo = 0;
    if (g < 0 || f0 >= TC) {
        o.kn = 0;
        o.ao = (unsigned)(lk * 4);
    } else {
        const long left = TC - f0;
        o.kn = (int)((left < G ? left : (long)G) / 16);
        o.ao = (unsigned)(((long)t.b * x_bstride + f0 + lk) * 4);
    }
    return o;
}

// byte offset the k loop requests for k-tile kt of a slab row (any kt: the request stream runs past a row's range, and past the tile at
// the end of a run); ok = the k-tile is data, otherwise the bytes of the row's first k-tile are re-loaded and cleared on use
__host__ __device__ __forceinline__ unsigned b3_shared_load_offset(const B3SharedRow& row, int kt, bool& ok) {
    ok = (unsigned)kt < (unsigned)row.kn;
    return row.ao + (ok ? (unsigned)kt : 0u) * 64u;
}

// plane pairs of the six products in the order they are accumulated (smallest terms first): A-side plane, B-side plane
#define B3_QA {2, 0, 1, 1, 0, 0}
#define B3_QB {0, 2, 1, 0, 1, 0}

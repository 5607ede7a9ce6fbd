// Small-batch decode GEMV on MXFP4 weights: y[b][n] = (res +) (bias +) sum_k P(x)[b][k] * dec(q[n][k]) * 2^e[n][k / 32], q OCP e2m1
// codes packed two per byte [N][K / 2] (even k in the low nibble), one power-of-two scale byte e + 127 per block of 32 k
// [N][K / 32], activations and accumulation fp32 -- weight-only storage, a quarter of the bytes of lm_step.hip's bf16 GEMV.
// code * 2^e is exactly a bf16 number, so the result differs from the bf16 GEMV on the dequantised weights by summation order only.
// The schedules are the templates of lm_gemv_quant.h; here are the format (W4Chunk and its trait Mxfp4Blocks), the choice of
// schedule per shape, and the quantiser (bf16 rows -> codes + scale bytes), run once when a model is loaded.
//
// Lane map: a 16-byte non-temporal load holds 32 consecutive k = ONE scale block, so a wave covers 2048 k of a row per load and lane
// l multiplies k = c * 2048 + 32 l + (0..31) of chunk c with the scale byte [n][c * 64 + l] (64 lanes: 64 contiguous bytes).  Read
// from an LDS stage in k order that would be eight ds_read_b128 per lane at a lane stride of 128 bytes, so the staged activations
// are PERMUTED: element k of chunk c lives at c * 2048 + 256 * ((k / 4) % 8) + 4 * ((k / 32) % 64) + k % 4, and the j-th read of every
// lane is 16 bytes at a lane stride of 16 bytes.  Decode: v_cvt_scalef32_pk_f32_fp4 (two codes of one byte times the fp32 scale
// 2^e, exact), then the packed fp32 FMA in k order: 16 converts + 16 packed FMAs per 16 bytes.
#include "lm_gemv_quant.h"

namespace {

// 32 consecutive k of one weight row (one scale block): 16 bytes of e2m1 codes and the block's scale byte
struct W4Chunk {
    u32x4 v;
    unsigned sb;
    __device__ __forceinline__ void zero() { v = u32x4{0u, 0u, 0u, 0u}; sb = 127u; }
    // row = the row's first block in the [N][K / 32] table, k = the lane's first k of the chunk; a block's codes are the 16 bytes at 16 * block
    __device__ __forceinline__ void load(const GemvQuantParams& p, long row, int k) {
        const long blk = row + (k >> 5);
        v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.q + blk * 16));
        sb = static_cast<const unsigned char*>(p.scale)[blk];
    }
    // a + 2^e * sum_i w[i] * x[i / 4][i % 4] (nibble i of the chunk is k + i: byte i / 2, even i low; little endian words, so word w
    // holds k + 8 w .. 8 w + 7 and byte b of it the pair k + 8 w + 2 b, + 1).  The convert yields the two weights of a byte already
    // scaled, so the sum runs as TWO chains (even / odd k) on the packed fp32 FMA, joined once per chunk.  The scale byte is >= 2
    // (e >= -125), so 2^e is a normal fp32 and code * 2^e >= 2^-126 is exact.
    __device__ __forceinline__ float dot(const f32x4 (&x)[8], float a) const {
        const float sc = __uint_as_float(sb << 23);
        f32x2 s = {a, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x2 w0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v[j], sc, 0), w1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v[j], sc, 1);
            const f32x2 w2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v[j], sc, 2), w3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v[j], sc, 3);
            s = __builtin_elementwise_fma(w0, __builtin_shufflevector(x[2 * j], x[2 * j], 0, 1), s);
            s = __builtin_elementwise_fma(w1, __builtin_shufflevector(x[2 * j], x[2 * j], 2, 3), s);
            s = __builtin_elementwise_fma(w2, __builtin_shufflevector(x[2 * j + 1], x[2 * j + 1], 0, 1), s);
            s = __builtin_elementwise_fma(w3, __builtin_shufflevector(x[2 * j + 1], x[2 * j + 1], 2, 3), s);
        }
        return s[0] + s[1];
    }
};

// the format trait of lm_gemv_quant.h: the scale is per block and applied inside dot()
struct Mxfp4Blocks {
    using Chunk = W4Chunk;
    static constexpr int K_PER_LOAD = 2048, K_PER_LANE = 32, XV = 8;
    static constexpr bool ROW_SCALE = false;
    static __device__ __forceinline__ int row_stride(int K) { return K >> 5; }
    static __device__ __forceinline__ int xs_slot(int k) { return (k & ~2047) | (((k >> 2) & 7) << 8) | (((k >> 5) & 63) << 2) | (k & 3); }
    static __device__ __forceinline__ void read_x(const float* xb, f32x4 (&x)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const f32x4*>(xb + 256 * j);
    }
};

// One thread per block of 32 weights: amax over the bf16 magnitudes (as integers: finite bf16 magnitudes order like their bit
// patterns), the exponent e = smallest integer with amax / 2^e <= 6 from the exponent and mantissa bits (6 = 1.5 * 2^2: a normalised
// amax 1.m * 2^t takes e = t - 2 if 1.m <= 1.5, else t - 1), clamped below at -125 (then 2^e and every code * 2^e are normal
// numbers; a clamped block simply uses smaller codes), every element scaled exactly (ldexpf) and rounded to nearest on the e2m1
// grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the code with an even mantissa bit: the grid's midpoints 0.25, 1.25, 2.5, 5 round down,
// 0.75, 1.75, 3.5 round up.
__global__ __launch_bounds__(NT) void quant_blocks_mxfp4_kernel(const unsigned short* __restrict__ w, unsigned char* __restrict__ q,
                                                               unsigned char* __restrict__ scale, long blocks) {
    for (long blk = (long)blockIdx.x * NT + threadIdx.x; blk < blocks; blk += (long)gridDim.x * NT) {
        u32x4 in[4];             // 32 bf16
#pragma unroll
        for (int j = 0; j < 4; ++j) in[j] = *reinterpret_cast<const u32x4*>(w + blk * 32 + 8 * j);
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) m = max(m, max(in[j][i] & 0x7fffu, (in[j][i] >> 16) & 0x7fffu));
        int e = 0;
        if (m) {
            int E = (int)(m >> 7), M = (int)(m & 0x7fu);          // biased exponent, 7 mantissa bits
            if (E == 0) {                                         // bf16 subnormal M * 2^-133: normalise
                const int top = 31 - __clz(M);
                M = (M << (7 - top)) & 0x7f;
                E = top - 6;
            }
            e = max(E - 127 - (M <= 64 ? 2 : 1), -125);
        }
        u32x4 out;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned word = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {                         // element 8 j + i: nibble i of word j
                const unsigned u = (i & 1 ? in[j][i >> 1] & 0xffff0000u : in[j][i >> 1] << 16);
                const float a = ldexpf(__uint_as_float(u & 0x7fffffffu), -e);      // exact; <= 6
                const unsigned code = (unsigned)(a > 0.25f) + (unsigned)(a >= 0.75f) + (unsigned)(a > 1.25f) + (unsigned)(a >= 1.75f) +
                                      (unsigned)(a > 2.5f) + (unsigned)(a >= 3.5f) + (unsigned)(a > 5.0f);
                word |= (code | ((u >> 28) & 8u)) << (4 * i);
            }
            out[j] = word;
        }
        *reinterpret_cast<u32x4*>(q + blk * 16) = out;
        scale[blk] = (unsigned char)(e + 127);
    }
}

}  // namespace

int rst_gemv_mxfp4w_supported_impl(int B, int N, int K) { return gemvq_supported<Mxfp4Blocks>(B, N, K, 32); }

// The rows schedule: a K <= 4096 row is at most 2 loads per lane here.  RPW = 8 rows per wave would keep fp8's 16 loads x 16 bytes per
// lane in flight, but measured slower than fewer rows and more workgroups on every per-layer shape: RPW = 2, and 4 =
// two (u, v) pairs with the gate.
int rst_launch_gemv_mxfp4w(const GemvQuantParams& p, hipStream_t stream) {
    size_t lds;
    if (const int err = gemvq_check<Mxfp4Blocks>(p, "gemv_mxfp4w", 32, &lds)) return err;
    const bool big = (long)p.N * p.K >= (1L << 24);
    // whole rows per wave, x requested before the weight stream: batch-1 layers of K <= 4096, RMSNorm (with or without the gate) or plain.
    // (Longer plain rows -- ffn-out -- take the LDS-staged schedule below: a K-split over the waves as in lm_gemv_fp8.hip measured slower.)
    if (big && p.B == 1 && p.K <= 4096 && (p.prologue == 1 || (p.prologue == 0 && !p.gate_out))) {
        if (p.gate_out) launch_gemvq<gemvq_rows_kernel<Mxfp4Blocks, 4, true, true>>(p, cap_grid(((long)p.N / 2 + 2 * GEMV_WAVES - 1) / (2 * GEMV_WAVES), 1024), lds, stream);
        else if (p.prologue == 1) launch_gemvq<gemvq_rows_kernel<Mxfp4Blocks, 2, false, true>>(p, cap_grid(((long)p.N + 2 * GEMV_WAVES - 1) / (2 * GEMV_WAVES), 1024), lds, stream);
        else launch_gemvq<gemvq_rows_kernel<Mxfp4Blocks, 2, false, false>>(p, cap_grid(((long)p.N + 2 * GEMV_WAVES - 1) / (2 * GEMV_WAVES), 1024), lds, stream);
        return rst_check_launch("gemv_mxfp4w");
    }
    // rows per wave: 4 when that still yields >= 2 workgroups per CU, else 2 (more workgroups -> more loads in flight)
    const bool rpw4 = !p.gate_out && ((long)p.N + 15) / 16 >= 512;
    const int rows_per_group = (rpw4 ? 4 : 2) * GEMV_WAVES;
    const long groups = p.gate_out ? ((long)p.N / 2 + GEMV_WAVES - 1) / GEMV_WAVES : ((long)p.N + rows_per_group - 1) / rows_per_group;
    launch_gemvq_general<Mxfp4Blocks>(p, rpw4, cap_grid(groups, lds > 48 * 1024 ? 512 : 768), lds, stream);
    return rst_check_launch("gemv_mxfp4w");
}

int rst_launch_quant_blocks_mxfp4(const unsigned short* w, unsigned char* q, unsigned char* scale, int N, int K, hipStream_t stream) {
    RST_REQUIRE(w && q && scale && N > 0 && K > 0 && K % 32 == 0, "quant_blocks_mxfp4: bad arguments (N=%d K=%d; K must be a multiple of 32)", N, K);
    RST_REQUIRE(((uintptr_t)w % 16) == 0 && ((uintptr_t)q % 16) == 0, "quant_blocks_mxfp4: pointers must be 16-byte aligned");
    const long blocks = (long)N * (K / 32);
    hipLaunchKernelGGL(quant_blocks_mxfp4_kernel, dim3(cap_grid((blocks + NT - 1) / NT, 65536)), dim3(NT), 0, stream, w, q, scale, blocks);
    return rst_check_launch("quant_blocks_mxfp4");
}

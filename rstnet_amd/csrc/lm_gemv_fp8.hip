// Small-batch decode GEMV on fp8 weights: y[b][n] = (res +) (bias +) s_n * sum_k P(x)[b][k] * q[n][k], q OCP e4m3fn bytes [N][K],
// s_n = 2^e_n one power-of-two scale per row (fp32), activations and accumulation fp32 -- weight-only storage, half the bytes of
// lm_step.hip's bf16 GEMV.  q * 2^e is exactly a bf16 number, so the result differs from the bf16 GEMV on the dequantised weights by
// summation order only.  The LDS-staged and the whole-rows-per-wave schedules are the templates of lm_gemv_quant.h; here are the
// format (W8Chunk and its trait Fp8Rows), the K-split schedule that only fp8 has, the choice of schedule per shape, and the
// quantiser (bf16 rows -> bytes + scales), run once when a model is loaded.
//
// Lane map: a 16-byte non-temporal load holds 16 consecutive k, so a wave covers 1024 k of a row per load (512 for bf16) and
// lane l multiplies k = c * 1024 + 16 l + (0..15) of chunk c.  Read naively from an LDS stage in k order that is four ds_read_b128
// per lane at a lane stride of 64 bytes (four-way bank conflicts), so the staged activations are PERMUTED: element k of chunk c
// lives at c * 1024 + 256 * ((k / 4) % 4) + 4 * ((k / 16) % 64) + k % 4, and the j-th read of every lane is 16 bytes at a lane stride
// of 16 bytes.  Decode: v_cvt_pk_f32_fp8 (two bytes per instruction, exact), then fmaf in k order: 8 converts + 16 FMAs per 16 bytes.
#include "lm_gemv_quant.h"

namespace {

// 16 consecutive k of one weight row: 16 e4m3 bytes
struct W8Chunk {
    u32x4 v;
    __device__ __forceinline__ void zero() { v = u32x4{0u, 0u, 0u, 0u}; }
    // row = the row's first byte, k = the lane's first k of the chunk
    __device__ __forceinline__ void load(const GemvQuantParams& p, long row, int k) {
        v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.q + row + k));
    }
    // a + sum_i w[i] * x[i / 4][i % 4] (byte i of the chunk is k + i: little endian words).  v_cvt_pk_f32_fp8 yields two weights, so
    // the sum runs as TWO chains (even / odd k) on the packed fp32 FMA (v_pk_fma_f32: 8 converts + 8 packed FMAs + 1 add per 16 bytes,
    // the instruction count of the bf16 chunk's 8 shifts + 8 FMAs), joined once per chunk.
    __device__ __forceinline__ float dot(const f32x4 (&x)[4], float a) const {
        f32x2 s = {a, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(v[j], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(v[j], true);
            s = __builtin_elementwise_fma(lo, __builtin_shufflevector(x[j], x[j], 0, 1), s);
            s = __builtin_elementwise_fma(hi, __builtin_shufflevector(x[j], x[j], 2, 3), s);
        }
        return s[0] + s[1];
    }
};

// the format trait of lm_gemv_quant.h: one fp32 scale per row, applied to the reduced sum
struct Fp8Rows {
    using Chunk = W8Chunk;
    static constexpr int K_PER_LOAD = 1024, K_PER_LANE = 16, XV = 4;
    static constexpr bool ROW_SCALE = true;
    static __device__ __forceinline__ int row_stride(int K) { return K; }
    static __device__ __forceinline__ const float* row_scales(const GemvQuantParams& p) { return static_cast<const float*>(p.scale); }
    static __device__ __forceinline__ int xs_slot(int k) { return (k & ~1023) | (((k >> 2) & 3) << 8) | (((k >> 4) & 63) << 2) | (k & 3); }
    static __device__ __forceinline__ void read_x(const float* xb, f32x4 (&x)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = *reinterpret_cast<const f32x4*>(xb + 256 * j);
    }
};

// Batch-1 GEMV on a plain activation vector (out-proj, ffn-out; gemv_ksplit_kernel of lm_step.hip): K split over the four waves, wave w
// takes the 1024-k chunks c = w, w + 4, ... of RW = 8 rows, the 16 activations a lane multiplies come straight from global memory
// (L2) into registers -- no LDS stage, no barrier in front of the weight stream.  Two chunks in flight per row; at K = 4096 a wave
// owns ONE chunk (bf16: two), so only 8 loads per lane are in flight there.  The four partial sums of a row are added in wave order.
template <int RW>
__global__ __launch_bounds__(NT) void gemv8_ksplit_kernel(const GemvQuantParams p) {
    __shared__ float part[GEMV_WAVES][RW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.K, nchunks = (K + 1023) >> 10;
    const int kl = lane * 16;
    const int groups = (p.N + RW - 1) / RW;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int n0 = grp * RW;
        long wrow[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) wrow[r] = (long)min(n0 + r, p.N - 1) * K;
        float acc[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[r] = 0.f;
        W8Chunk wa[RW], wb[RW];
        f32x4 xa[4], xb[4];
        auto issue = [&](W8Chunk (&w)[RW], f32x4 (&x)[4], int c) {
            const int kk = (c << 10) + kl;
            const bool ok = c < nchunks && kk < K;
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = ok ? *reinterpret_cast<const f32x4*>(p.x + kk + 4 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                if (ok) w[r].load(p, wrow[r], kk);
                else w[r].zero();
            }
        };
        issue(wa, xa, wave);
        for (int c = wave; c < nchunks; c += 2 * GEMV_WAVES) {
            issue(wb, xb, c + GEMV_WAVES);
#pragma unroll
            for (int r = 0; r < RW; ++r) acc[r] = wa[r].dot(xa, acc[r]);
            issue(wa, xa, c + 2 * GEMV_WAVES);
#pragma unroll
            for (int r = 0; r < RW; ++r) acc[r] = wb[r].dot(xb, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[r] = wave_sum_fast(acc[r]);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < RW; ++r) part[wave][r] = acc[r];
        }
        __syncthreads();
        if (tid < RW && n0 + tid < p.N) {
            const int n = n0 + tid;
            float sb = (((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]) * Fp8Rows::row_scales(p)[n];
            if (p.bias) sb += p.bias[n];
            p.y[n] = p.res ? p.res[n] + sb : sb;
        }
        __syncthreads();          // part is rewritten by the next group
    }
}

// One workgroup per row: amax over the bf16 magnitudes (as integers: finite bf16 magnitudes order like their bit patterns), the
// exponent e = smallest integer with amax / 2^e <= 448 from the exponent and mantissa bits (448 = 1.75 * 2^8: a normalised amax
// 1.m * 2^t takes e = t - 8 if 1.m <= 1.75, else t - 7), then every element scaled exactly (ldexpf) and rounded to nearest even.
__global__ __launch_bounds__(NT) void quant_rows_fp8_kernel(const unsigned short* __restrict__ w, unsigned char* __restrict__ q,
                                                           float* __restrict__ scale, int N, int K) {
    __shared__ unsigned red[GEMV_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        const unsigned short* wr = w + (long)n * K;
        unsigned m = 0;
        for (int k = tid; k < K; k += NT) m = max(m, (unsigned)wr[k] & 0x7fffu);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
        __syncthreads();          // red is still read by the previous row
        if (lane == 0) red[wave] = m;
        __syncthreads();
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        int e = 0;
        if (m) {
            int E = (int)(m >> 7), M = (int)(m & 0x7fu);          // biased exponent, 7 mantissa bits
            if (E == 0) {                                         // bf16 subnormal M * 2^-133: normalise
                const int top = 31 - __clz(M);
                M = (M << (7 - top)) & 0x7f;
                E = top - 6;
            }
            e = E - 127 - (M <= 96 ? 8 : 7);
        }
        if (tid == 0) scale[n] = __uint_as_float(e >= -126 ? (unsigned)(e + 127) << 23 : 1u << (e + 149));
        unsigned char* qr = q + (long)n * K;
        for (int k = tid; k < K; k += NT) {
            const unsigned u = (unsigned)wr[k] << 16;
            const float v = ldexpf(__uint_as_float(u & 0x7fffffffu), -e);      // exact; |v| <= 448
            const unsigned a = __float_as_uint(v);
            unsigned code;
            if (a >= 0x3C800000u) {                               // >= 2^-6: an e4m3 normal; RNE on bit 20, the carry may enter the exponent
                code = ((a + 0x7FFFFu + ((a >> 20) & 1u)) >> 20) - (120u << 3);
            } else {                                              // e4m3 subnormals are multiples of 2^-9 (8 = the smallest normal)
                code = (unsigned)__float2int_rn(v * 512.0f);
            }
            qr[k] = (unsigned char)(code | ((u >> 24) & 0x80u));
        }
    }
}

}  // namespace

int rst_gemv_fp8w_supported_impl(int B, int N, int K) { return gemvq_supported<Fp8Rows>(B, N, K, 16); }

// The rows schedule takes RPW = 4 rows per wave: a K <= 4096 row is at most 4 loads per lane, and 4 rows keep the bf16 form's 16 loads
// x 16 bytes per lane in flight.  It serves the batch-1 RMSNorm layers (qkv, ffn-in) and plain layers of many rows of K <= 4096 (text
// head, stacked depformer_in), where the K-split leaves a wave one chunk per row group and pays a barrier pair and eight reductions
// per 32 KB.
int rst_launch_gemv_fp8w(const GemvQuantParams& p, hipStream_t stream) {
    size_t lds;
    if (const int err = gemvq_check<Fp8Rows>(p, "gemv_fp8w", 16, &lds)) return err;
    const bool big = (long)p.N * p.K >= (1L << 24);
    // whole rows per wave, x requested before the weight stream: the batch-1 RMSNorm layers, and plain layers of >= 8192 rows of K <= 4096
    const bool plain_rows = p.prologue == 0 && !p.gate_out && p.N >= 8192;
    if (big && p.B == 1 && p.K <= 4096 && (p.prologue == 1 || plain_rows)) {
        const long groups = p.gate_out ? ((long)p.N / 2 + 2 * GEMV_WAVES - 1) / (2 * GEMV_WAVES) : ((long)p.N + 4 * GEMV_WAVES - 1) / (4 * GEMV_WAVES);
        const unsigned grid = cap_grid(groups, 1024);
        if (p.prologue == 0) launch_gemvq<gemvq_rows_kernel<Fp8Rows, 4, false, false>>(p, grid, lds, stream);
        else if (p.gate_out) launch_gemvq<gemvq_rows_kernel<Fp8Rows, 4, true, true>>(p, grid, lds, stream);
        else launch_gemvq<gemvq_rows_kernel<Fp8Rows, 4, false, true>>(p, grid, lds, stream);
        return rst_check_launch("gemv_fp8w");
    }
    if (big && p.B == 1 && p.prologue == 0 && !p.gate_out && p.K >= 2048) {   // K split over the waves, activations in registers
        hipLaunchKernelGGL(gemv8_ksplit_kernel<8>, dim3(cap_grid(((long)p.N + 7) / 8, 1024)), dim3(NT), 0, stream, p);
        return rst_check_launch("gemv_fp8w");
    }
    // rows per wave: 4 when that still yields >= 2 workgroups per CU, else 2 (more workgroups -> more loads in flight)
    const bool rpw4 = !p.gate_out && ((long)p.N + 15) / 16 >= 512;
    const int rows_per_group = (rpw4 ? 4 : 2) * GEMV_WAVES;
    const long groups = p.gate_out ? ((long)p.N / 2 + GEMV_WAVES - 1) / GEMV_WAVES : ((long)p.N + rows_per_group - 1) / rows_per_group;
    launch_gemvq_general<Fp8Rows>(p, rpw4, cap_grid(groups, lds > 48 * 1024 ? 512 : 768), lds, stream);
    return rst_check_launch("gemv_fp8w");
}

int rst_launch_quant_rows_fp8(const unsigned short* w, unsigned char* q, float* scale, int N, int K, hipStream_t stream) {
    RST_REQUIRE(w && q && scale && N > 0 && K > 0, "quant_rows_fp8: bad arguments (N=%d K=%d)", N, K);
    hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3(cap_grid(N, 65536)), dim3(NT), 0, stream, w, q, scale, N, K);
    return rst_check_launch("quant_rows_fp8");
}

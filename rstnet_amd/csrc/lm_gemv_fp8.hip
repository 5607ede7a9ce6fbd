// Small-batch decode GEMV on fp8 weights: y[b][n] = (res +) (bias +) s_n * sum_k P(x)[b][k] * q[n][k], q OCP e4m3fn bytes [N][K],
// s_n = 2^e_n one power-of-two scale per row (fp32), activations and accumulation fp32 -- weight-only storage, half the bytes of
// lm_step.hip's bf16 GEMV, which this file mirrors schedule for schedule (it is a separate translation unit so that the bf16 objects
// stay bit-identical).  q * 2^e is exactly a bf16 number, so the result differs from the bf16 GEMV on the dequantised weights by
// summation order only.
//
// Lane map: a 16-byte non-temporal load now holds 16 consecutive k, so a wave covers 1024 k of a row per load (512 for bf16) and
// lane l multiplies k = c * 1024 + 16 l + (0..15) of chunk c.  Read naively from an LDS stage in k order that is four ds_read_b128
// per lane at a lane stride of 64 bytes (four-way bank conflicts), so the staged activations are PERMUTED: element k of chunk c
// lives at c * 1024 + 256 * ((k / 4) % 4) + 4 * ((k / 16) % 64) + k % 4, and the j-th read of every lane is 16 bytes at a lane stride
// of 16 bytes.  Decode: v_cvt_pk_f32_fp8 (two bytes per instruction, exact), then fmaf in k order: 8 converts + 16 FMAs per 16 bytes.
//
// Also here: the quantiser (bf16 rows -> bytes + scales), run once when a model is loaded.
#include "lm_common.h"

namespace {

constexpr int GEMV_WAVES = 4;
constexpr int NT = 64 * GEMV_WAVES;
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int xs_slot(int k) { return (k & ~1023) | (((k >> 2) & 3) << 8) | (((k >> 4) & 63) << 2) | (k & 3); }

// 16 consecutive k of one weight row: 16 e4m3 bytes
struct W8Chunk {
    u32x4 v;
    __device__ __forceinline__ void zero() { v = u32x4{0u, 0u, 0u, 0u}; }
    __device__ __forceinline__ void load(const unsigned char* q, long byte) {
        v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(q + byte));
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

// The general schedule (gemv_kernel of lm_step.hip): activations staged once per workgroup in LDS (permuted, see above), RPW rows per
// wave, the first weight chunk, the residual and the row scales of the first row group requested before the prologue, two chunks
// in flight per row in the loop.  xs holds [B][KS], KS = K rounded up to 1024; slots beyond K are never read.
template <int B, int RPW>
__global__ __launch_bounds__(NT) void gemv8_kernel(const GemvFp8Params p) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    __shared__ float red[GEMV_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.K, KS = (K + 1023) & ~1023;
    const int half = p.N / 2;
    const int groups = p.gate_out ? (half + GEMV_WAVES - 1) / GEMV_WAVES : (p.N + RPW * GEMV_WAVES - 1) / (RPW * GEMV_WAVES);
    // gate_out (RPW == 2): the wave's two rows are (n, N/2 + n) = (u_n, v_n) of a stacked gated layer, one output silu(u) * v
    auto row_of = [&](int grp, int r) {
        const int n = grp * GEMV_WAVES + wave;
        return p.gate_out ? r * half + min(n, half - 1) : min(n * RPW + r, p.N - 1);
    };
    W8Chunk wpre[RPW];
    float spre[RPW], rpre[RPW][B];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        wpre[r].zero();
        if (blockIdx.x < groups && lane * 16 < K) wpre[r].load(p.q, (long)row_of(blockIdx.x, r) * K + lane * 16);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        spre[r] = lane == 0 && blockIdx.x < groups ? p.scale[row_of(blockIdx.x, r)] : 0.f;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            rpre[r][b] = 0.f;
            const int n = (blockIdx.x * GEMV_WAVES + wave) * RPW + r;
            if (p.res && !p.gate_out && lane == 0 && n < p.N) rpre[r][b] = p.res[(long)b * p.ldy + n];
        }
    }

    // ---- prologue: stage the activation vector(s) in LDS
    if (p.prologue == 1) {           // RMSNorm: x * alpha * rsqrt(eps + mean(x^2))   (modules/transformer.py:34-46)
        for (int b = 0; b < B; ++b) {
            constexpr int XR = 16;   // elements kept in registers between the two passes (K <= 4096); the rest is re-read
            float xr[XR];
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < XR; ++i) {
                const int k = tid + i * NT;
                xr[i] = k < K ? p.x[(long)b * p.ldx + k] : 0.f;
                s = fmaf(xr[i], xr[i], s);
            }
            for (int k = tid + XR * NT; k < K; k += NT) { const float v = p.x[(long)b * p.ldx + k]; s = fmaf(v, v, s); }
            s = wave_sum(s);
            __syncthreads();
            if (lane == 0) red[wave] = s;
            __syncthreads();
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < GEMV_WAVES; ++w) tot += red[w];
            const float r = 1.0f / sqrtf(p.eps + tot / (float)K);
#pragma unroll
            for (int i = 0; i < XR; ++i) {
                const int k = tid + i * NT;
                if (k < K) xs[b * KS + xs_slot(k)] = xr[i] * (p.alpha[k] * r);
            }
            for (int k = tid + XR * NT; k < K; k += NT) xs[b * KS + xs_slot(k)] = p.x[(long)b * p.ldx + k] * (p.alpha[k] * r);
        }
    } else if (p.prologue == 2) {    // SiLU gate: x holds [B][2K] = [u ; v], xs = silu(u) * v   (modules/gating.py:12-22)
        for (int b = 0; b < B; ++b)
            for (int k = tid; k < K; k += NT) xs[b * KS + xs_slot(k)] = silu(p.x[(long)b * p.ldx + k]) * p.x[(long)b * p.ldx + K + k];
    } else {
        for (int b = 0; b < B; ++b)
            for (int k = tid; k < K; k += NT) xs[b * KS + xs_slot(k)] = p.x[(long)b * p.ldx + k];
    }
    __syncthreads();

    // ---- row groups, grid-strided: RPW rows per wave, 16 bytes (16 k) per lane per row per iteration, two iterations in flight
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int n0 = (grp * GEMV_WAVES + wave) * RPW;
        float acc[RPW][B];
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int b = 0; b < B; ++b) acc[r][b] = 0.f;
        long wrow[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) wrow[r] = (long)row_of(grp, r) * K;
        auto fma16 = [&](const W8Chunk (&wv)[RPW], int k) {      // k = c * 1024 + 16 * lane
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const float* xb = xs + b * KS + (k & ~1023) + lane * 4;
                const f32x4 x[4] = {*reinterpret_cast<const f32x4*>(xb), *reinterpret_cast<const f32x4*>(xb + 256),
                                    *reinterpret_cast<const f32x4*>(xb + 512), *reinterpret_cast<const f32x4*>(xb + 768)};
#pragma unroll
                for (int r = 0; r < RPW; ++r) acc[r][b] = wv[r].dot(x, acc[r][b]);
            }
        };
        const bool first = grp == (int)blockIdx.x;
        int k = lane * 16;
        if (first && k < K) {        // the prefetched chunk
            fma16(wpre, k);
            k += 1024;
        }
        for (; k + 1024 < K; k += 2048) {
            W8Chunk wa[RPW], wb[RPW];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                wa[r].load(p.q, wrow[r] + k);
                wb[r].load(p.q, wrow[r] + k + 1024);
            }
            fma16(wa, k);
            fma16(wb, k + 1024);
        }
        if (k < K) {
            W8Chunk wa[RPW];
#pragma unroll
            for (int r = 0; r < RPW; ++r) wa[r].load(p.q, wrow[r] + k);
            fma16(wa, k);
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int b = 0; b < B; ++b) acc[r][b] = wave_sum(acc[r][b]);
        if (lane != 0) continue;
        float sc[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) sc[r] = first ? spre[r] : p.scale[row_of(grp, r)];
        if (p.gate_out) {
            const int n = grp * GEMV_WAVES + wave;
            if (n < half)
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    float u = acc[0][b] * sc[0], v = acc[RPW - 1][b] * sc[RPW - 1];
                    if (p.bias) { u += p.bias[n]; v += p.bias[half + n]; }
                    p.y[(long)b * p.ldy + n] = silu(u) * v;
                }
            continue;
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const int n = n0 + r;
                if (n < p.N) {
                    const long o = (long)b * p.ldy + n;
                    float sb = acc[r][b] * sc[r];
                    if (p.bias) sb += p.bias[n];
                    p.y[o] = p.res ? (first ? rpre[r][b] : p.res[o]) + sb : sb;
                }
            }
    }
}

// Batch-1 RMSNorm -> GEMV for the large layers (qkv, ffn-in; gemv_norm_kernel of lm_step.hip): x and alpha are requested FIRST, then
// every weight byte of the wave's rows, and the norm runs on data that arrives ahead of the weights.  NORM = false: the same schedule
// on a plain vector (text head, stacked depformer_in: many rows of K = 4096, where the K-split schedule leaves a wave one chunk per
// row group and pays a barrier pair and eight reductions per 32 KB).  A K <= 4096 row is at most
// PRE = 4 chunks here (8 for bf16), so a wave takes RPW = 4 rows instead of 2 to keep the same 16 loads x 16 bytes per lane in
// flight.  GATE: the wave's rows are two (u, v) pairs (n, N/2 + n), (n + 1, N/2 + n + 1).
template <bool GATE, bool NORM>
__global__ __launch_bounds__(NT) void gemv8_norm_kernel(const GemvFp8Params p) {
    constexpr int RPW = 4, PRE = 4, XR = 16;
    extern __shared__ __attribute__((aligned(16))) float xs[];   // [KS] permuted
    __shared__ float red[GEMV_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.K, half = p.N / 2;
    const int groups = GATE ? (half + 2 * GEMV_WAVES - 1) / (2 * GEMV_WAVES) : (p.N + RPW * GEMV_WAVES - 1) / (RPW * GEMV_WAVES);
    const int kl = lane * 16;

    float xa[XR], al[XR];            // K <= XR * NT = 4096 (launch check)
#pragma unroll
    for (int i = 0; i < XR; ++i) {
        const int k = tid + i * NT;
        xa[i] = k < K ? p.x[k] : 0.f;
        al[i] = NORM && k < K ? p.alpha[k] : 0.f;
    }
    W8Chunk buf[PRE][RPW];
    float sc[RPW];
    auto row_of = [&](int grp, int r) {
        const int n = grp * GEMV_WAVES + wave;
        return GATE ? (r & 1) * half + min(2 * n + (r >> 1), half - 1) : min(n * RPW + r, p.N - 1);
    };
    auto issue = [&](int grp) {      // all chunks of the wave's rows, then their scales
#pragma unroll
        for (int j = 0; j < PRE; ++j)
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int kk = (j << 10) + kl;
                if (kk < K) buf[j][r].load(p.q, (long)row_of(grp, r) * K + kk);
                else buf[j][r].zero();
            }
#pragma unroll
        for (int r = 0; r < RPW; ++r) sc[r] = p.scale[row_of(grp, r)];
    };
    issue(blockIdx.x < groups ? blockIdx.x : 0);

    if (NORM) {                      // RMSNorm: x * alpha * rsqrt(eps + mean(x^2))   (modules/transformer.py:34-46)
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < XR; ++i) s = fmaf(xa[i], xa[i], s);
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < GEMV_WAVES; ++w) tot += red[w];
        const float r = 1.0f / sqrtf(p.eps + tot / (float)K);
#pragma unroll
        for (int i = 0; i < XR; ++i) xa[i] *= al[i] * r;
    }
#pragma unroll
    for (int i = 0; i < XR; ++i) {
        const int k = tid + i * NT;
        if (k < K) xs[xs_slot(k)] = xa[i];
    }
    __syncthreads();

    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        if (grp != (int)blockIdx.x) issue(grp);
        float acc[RPW] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < PRE; ++j) {
            if ((j << 10) + kl < K) {
                const float* xb = xs + (j << 10) + lane * 4;
                const f32x4 x[4] = {*reinterpret_cast<const f32x4*>(xb), *reinterpret_cast<const f32x4*>(xb + 256),
                                    *reinterpret_cast<const f32x4*>(xb + 512), *reinterpret_cast<const f32x4*>(xb + 768)};
#pragma unroll
                for (int r = 0; r < RPW; ++r) acc[r] = buf[j][r].dot(x, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) acc[r] = wave_sum_fast(acc[r]);
        if (lane != 0) continue;
        const int n = grp * GEMV_WAVES + wave;
        if (GATE) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int o = 2 * n + h;
                if (o < half) {
                    float u = acc[2 * h] * sc[2 * h], v = acc[2 * h + 1] * sc[2 * h + 1];
                    if (p.bias) { u += p.bias[o]; v += p.bias[half + o]; }
                    p.y[o] = silu(u) * v;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int o = n * RPW + r;
                if (o < p.N) {
                    float sb = acc[r] * sc[r];
                    if (p.bias) sb += p.bias[o];
                    p.y[o] = p.res ? p.res[o] + sb : sb;
                }
            }
        }
    }
}

// Batch-1 GEMV on a plain activation vector (out-proj, ffn-out; gemv_ksplit_kernel of lm_step.hip): K split over the four waves, wave w
// takes the 1024-k chunks c = w, w + 4, ... of RW = 8 rows, the 16 activations a lane multiplies come straight from global memory
// (L2) into registers -- no LDS stage, no barrier in front of the weight stream.  Two chunks in flight per row; at K = 4096 a wave
// owns ONE chunk (bf16: two), so only 8 loads per lane are in flight there.  The four partial sums of a row are added in wave order.
template <int RW>
__global__ __launch_bounds__(NT) void gemv8_ksplit_kernel(const GemvFp8Params p) {
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
                if (ok) w[r].load(p.q, wrow[r] + kk);
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
            float sb = (((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]) * p.scale[n];
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

// the opt-in to more than 64 KiB of dynamic LDS is per kernel and per device: one flag per instantiation
template <auto KERN>
void launch8(const GemvFp8Params& p, unsigned grid, size_t shmem, hipStream_t stream) {
    static RstOncePerDevice attr_once;
    if (attr_once.first()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipGetLastError();
    }
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(NT), shmem, stream, p);
}

}  // namespace

// B <= 4, K a multiple of 16 (a lane's 16-byte load must not straddle a row) and B * roundup(K, 1024) fp32 within the 128 KiB stage
int rst_gemv_fp8w_supported_impl(int B, int N, int K) {
    return B >= 1 && B <= 4 && N > 0 && K > 0 && K % 16 == 0 && (long)B * ((K + 1023) & ~1023) <= 32768;
}

int rst_launch_gemv_fp8w(const GemvFp8Params& p, hipStream_t stream) {
    RST_REQUIRE(p.B >= 1 && p.B <= 4 && p.N > 0 && p.K > 0 && p.K % 16 == 0, "gemv_fp8w: need 1 <= B <= 4 and K %% 16 == 0 (B=%d K=%d)", p.B, p.K);
    RST_REQUIRE(p.x && p.q && p.scale && p.y, "gemv_fp8w: null pointer");
    RST_REQUIRE(p.prologue >= 0 && p.prologue <= 2 && (p.prologue != 1 || p.alpha), "gemv_fp8w: prologue must be 0 (none), 1 (RMSNorm, needs alpha) or 2 (SiLU gate)");
    RST_REQUIRE(((uintptr_t)p.q % 16) == 0 && ((uintptr_t)p.x % 16) == 0, "gemv_fp8w: pointers must be 16-byte aligned");
    RST_REQUIRE(!p.gate_out || (p.N % 2 == 0 && !p.res), "gemv_fp8w: gate_out needs an even N and no residual");
    RST_REQUIRE(p.ldx >= (p.prologue == 2 ? 2 * p.K : p.K) && p.ldy >= (p.gate_out ? p.N / 2 : p.N), "gemv_fp8w: ldx / ldy too small (ldx=%d ldy=%d)", p.ldx, p.ldy);
    const int KS = (p.K + 1023) & ~1023;
    const size_t lds = (size_t)p.B * KS * sizeof(float);
    RST_REQUIRE(lds <= 128 * 1024, "gemv_fp8w: B * roundup(K, 1024) = %d floats do not fit the activation stage (32768)", p.B * KS);
    const bool big = (long)p.N * p.K >= (1L << 24);
    // whole rows per wave, x requested before the weight stream: the batch-1 RMSNorm layers, and plain layers of >= 8192 rows of K <= 4096
    const bool plain_rows = p.prologue == 0 && !p.gate_out && p.N >= 8192;
    if (big && p.B == 1 && p.K <= 4096 && (p.prologue == 1 || plain_rows)) {
        const long groups = p.gate_out ? ((long)p.N / 2 + 2 * GEMV_WAVES - 1) / (2 * GEMV_WAVES) : ((long)p.N + 4 * GEMV_WAVES - 1) / (4 * GEMV_WAVES);
        const unsigned grid = cap_grid(groups, 1024);
        if (p.prologue == 0) launch8<gemv8_norm_kernel<false, false>>(p, grid, lds, stream);
        else if (p.gate_out) launch8<gemv8_norm_kernel<true, true>>(p, grid, lds, stream);
        else launch8<gemv8_norm_kernel<false, true>>(p, grid, lds, stream);
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
    const unsigned grid = cap_grid(groups, lds > 48 * 1024 ? 512 : 768);
    switch (p.B * 2 + (rpw4 ? 1 : 0)) {
        case 2: launch8<gemv8_kernel<1, 2>>(p, grid, lds, stream); break;
        case 3: launch8<gemv8_kernel<1, 4>>(p, grid, lds, stream); break;
        case 4: launch8<gemv8_kernel<2, 2>>(p, grid, lds, stream); break;
        case 5: launch8<gemv8_kernel<2, 4>>(p, grid, lds, stream); break;
        case 6: launch8<gemv8_kernel<3, 2>>(p, grid, lds, stream); break;
        case 7: launch8<gemv8_kernel<3, 4>>(p, grid, lds, stream); break;
        case 8: launch8<gemv8_kernel<4, 2>>(p, grid, lds, stream); break;
        default: launch8<gemv8_kernel<4, 4>>(p, grid, lds, stream); break;
    }
    return rst_check_launch("gemv_fp8w");
}

int rst_launch_quant_rows_fp8(const unsigned short* w, unsigned char* q, float* scale, int N, int K, hipStream_t stream) {
    RST_REQUIRE(w && q && scale && N > 0 && K > 0, "quant_rows_fp8: bad arguments (N=%d K=%d)", N, K);
    hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3(cap_grid(N, 65536)), dim3(NT), 0, stream, w, q, scale, N, K);
    return rst_check_launch("quant_rows_fp8");
}

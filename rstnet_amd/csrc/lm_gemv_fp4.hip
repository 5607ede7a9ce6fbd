// Small-batch decode GEMV on MXFP4 weights: y[b][n] = (res +) (bias +) sum_k P(x)[b][k] * dec(q[n][k]) * 2^e[n][k / 32], q OCP e2m1
// codes packed two per byte [N][K / 2] (even k in the low nibble), one power-of-two scale byte e + 127 per block of 32 k
// [N][K / 32], activations and accumulation fp32 -- weight-only storage, a quarter of the bytes of lm_step.hip's bf16 GEMV.  The
// file-for-file sibling of lm_gemv_fp8.hip (a separate translation unit so that the bf16 and fp8 objects stay bit-identical).
// code * 2^e is exactly a bf16 number, so the result differs from the bf16 GEMV on the dequantised weights by summation order only.
//
// Lane map: a 16-byte non-temporal load holds 32 consecutive k = ONE scale block, so a wave covers 2048 k of a row per load and lane
// l multiplies k = c * 2048 + 32 l + (0..31) of chunk c with the scale byte [n][c * 64 + l] (64 lanes: 64 contiguous bytes).  Read
// from an LDS stage in k order that would be eight ds_read_b128 per lane at a lane stride of 128 bytes, so the staged activations
// are PERMUTED: element k of chunk c lives at c * 2048 + 256 * ((k / 4) % 8) + 4 * ((k / 32) % 64) + k % 4, and the j-th read of every
// lane is 16 bytes at a lane stride of 16 bytes.  Decode: v_cvt_scalef32_pk_f32_fp4 (two codes of one byte times the fp32 scale
// 2^e, exact), then the packed fp32 FMA in k order: 16 converts + 16 packed FMAs per 16 bytes.
//
// Also here: the quantiser (bf16 rows -> codes + scale bytes), run once when a model is loaded.
#include "lm_common.h"

namespace {

constexpr int GEMV_WAVES = 4;
constexpr int NT = 64 * GEMV_WAVES;
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int xs_slot(int k) { return (k & ~2047) | (((k >> 2) & 7) << 8) | (((k >> 5) & 63) << 2) | (k & 3); }

// 32 consecutive k of one weight row (one scale block): 16 bytes of e2m1 codes and the block's scale byte
struct W4Chunk {
    u32x4 v;
    unsigned sb;
    __device__ __forceinline__ void zero() { v = u32x4{0u, 0u, 0u, 0u}; sb = 127u; }
    // blk = the block's index in the [N][K / 32] table; its codes are the 16 bytes at 16 * blk
    __device__ __forceinline__ void load(const unsigned char* q, const unsigned char* scale, long blk) {
        v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(q + blk * 16));
        sb = scale[blk];
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

// the eight 16-byte reads of a lane's 32 staged activations of the chunk at xb (= stage + chunk base + 4 * lane)
__device__ __forceinline__ void read_x32(const float* xb, f32x4 (&x)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const f32x4*>(xb + 256 * j);
}

// The general schedule (gemv8_kernel of lm_gemv_fp8.hip): activations staged once per workgroup in LDS (permuted, see above), RPW
// rows per wave, the first weight chunk (with its scale bytes) and the residual of the first row group requested before the
// prologue, two chunks in flight per row in the loop.  xs holds [B][KS], KS = K rounded up to 2048; slots beyond K are never read.
template <int B, int RPW>
__global__ __launch_bounds__(NT) void gemv4_kernel(const GemvFp4Params p) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    __shared__ float red[GEMV_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.K, KS = (K + 2047) & ~2047, KB = K >> 5;
    const int half = p.N / 2;
    const int groups = p.gate_out ? (half + GEMV_WAVES - 1) / GEMV_WAVES : (p.N + RPW * GEMV_WAVES - 1) / (RPW * GEMV_WAVES);
    // gate_out (RPW == 2): the wave's two rows are (n, N/2 + n) = (u_n, v_n) of a stacked gated layer, one output silu(u) * v
    auto row_of = [&](int grp, int r) {
        const int n = grp * GEMV_WAVES + wave;
        return p.gate_out ? r * half + min(n, half - 1) : min(n * RPW + r, p.N - 1);
    };
    W4Chunk wpre[RPW];
    float rpre[RPW][B];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        wpre[r].zero();
        if (blockIdx.x < groups && lane * 32 < K) wpre[r].load(p.q, p.scale, (long)row_of(blockIdx.x, r) * KB + lane);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
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

    // ---- row groups, grid-strided: RPW rows per wave, 16 bytes (32 k) per lane per row per iteration, two iterations in flight
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int n0 = (grp * GEMV_WAVES + wave) * RPW;
        float acc[RPW][B];
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int b = 0; b < B; ++b) acc[r][b] = 0.f;
        long wrow[RPW];              // first block of the row
#pragma unroll
        for (int r = 0; r < RPW; ++r) wrow[r] = (long)row_of(grp, r) * KB;
        auto fma32 = [&](const W4Chunk (&wv)[RPW], int k) {      // k = c * 2048 + 32 * lane
#pragma unroll
            for (int b = 0; b < B; ++b) {
                f32x4 x[8];
                read_x32(xs + b * KS + (k & ~2047) + lane * 4, x);
#pragma unroll
                for (int r = 0; r < RPW; ++r) acc[r][b] = wv[r].dot(x, acc[r][b]);
            }
        };
        const bool first = grp == (int)blockIdx.x;
        int k = lane * 32;
        if (first && k < K) {        // the prefetched chunk
            fma32(wpre, k);
            k += 2048;
        }
        for (; k + 2048 < K; k += 4096) {
            W4Chunk wa[RPW], wb[RPW];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                wa[r].load(p.q, p.scale, wrow[r] + (k >> 5));
                wb[r].load(p.q, p.scale, wrow[r] + ((k + 2048) >> 5));
            }
            fma32(wa, k);
            fma32(wb, k + 2048);
        }
        if (k < K) {
            W4Chunk wa[RPW];
#pragma unroll
            for (int r = 0; r < RPW; ++r) wa[r].load(p.q, p.scale, wrow[r] + (k >> 5));
            fma32(wa, k);
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int b = 0; b < B; ++b) acc[r][b] = wave_sum(acc[r][b]);
        if (lane != 0) continue;
        if (p.gate_out) {
            const int n = grp * GEMV_WAVES + wave;
            if (n < half)
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    float u = acc[0][b], v = acc[RPW - 1][b];
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
                    float sb = acc[r][b];
                    if (p.bias) sb += p.bias[n];
                    p.y[o] = p.res ? (first ? rpre[r][b] : p.res[o]) + sb : sb;
                }
            }
    }
}

// Batch-1 whole rows per wave for K <= 4096 (gemv8_norm_kernel of lm_gemv_fp8.hip): x (and alpha) are requested FIRST, then every
// weight byte and scale byte of the wave's rows, and the norm runs on data that arrives ahead of the weights.  NORM = false: the same
// schedule on a plain vector (out-proj, text head, stacked depformer_in).  A K <= 4096 row is at most PRE = 2 loads per lane here (4
// for fp8, 8 for bf16).  RPW = 8 rows per wave would keep fp8's 16 loads x 16 bytes per lane in flight, but measured slower than
// fewer rows and more workgroups on every per-layer shape: the launcher takes RPW = 2, and 4 = two (u, v) pairs
// (n, N/2 + n), (n + 1, N/2 + n + 1) with GATE.
template <int RPW, bool GATE, bool NORM>
__global__ __launch_bounds__(NT) void gemv4_rows_kernel(const GemvFp4Params p) {
    constexpr int PRE = 2, XR = 16, PPW = RPW / 2;
    extern __shared__ __attribute__((aligned(16))) float xs[];   // [KS] permuted
    __shared__ float red[GEMV_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.K, KB = K >> 5, half = p.N / 2;
    const int groups = GATE ? (half + PPW * GEMV_WAVES - 1) / (PPW * GEMV_WAVES) : (p.N + RPW * GEMV_WAVES - 1) / (RPW * GEMV_WAVES);
    const int kl = lane * 32;

    float xa[XR], al[XR];            // K <= XR * NT = 4096 (launch check)
#pragma unroll
    for (int i = 0; i < XR; ++i) {
        const int k = tid + i * NT;
        xa[i] = k < K ? p.x[k] : 0.f;
        al[i] = NORM && k < K ? p.alpha[k] : 0.f;
    }
    W4Chunk buf[PRE][RPW];
    auto row_of = [&](int grp, int r) {
        const int n = grp * GEMV_WAVES + wave;
        return GATE ? (r & 1) * half + min(PPW * n + (r >> 1), half - 1) : min(n * RPW + r, p.N - 1);
    };
    auto issue = [&](int grp) {      // all chunks of the wave's rows with their scale bytes
#pragma unroll
        for (int j = 0; j < PRE; ++j)
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int kk = (j << 11) + kl;
                if (kk < K) buf[j][r].load(p.q, p.scale, (long)row_of(grp, r) * KB + (kk >> 5));
                else buf[j][r].zero();
            }
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
        float acc[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) acc[r] = 0.f;
#pragma unroll
        for (int j = 0; j < PRE; ++j) {
            if ((j << 11) + kl < K) {
                f32x4 x[8];
                read_x32(xs + (j << 11) + lane * 4, x);
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
            for (int h = 0; h < PPW; ++h) {
                const int o = PPW * n + h;
                if (o < half) {
                    float u = acc[2 * h], v = acc[2 * h + 1];
                    if (p.bias) { u += p.bias[o]; v += p.bias[half + o]; }
                    p.y[o] = silu(u) * v;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int o = n * RPW + r;
                if (o < p.N) {
                    float sb = acc[r];
                    if (p.bias) sb += p.bias[o];
                    p.y[o] = p.res ? p.res[o] + sb : sb;
                }
            }
        }
    }
}

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

// the opt-in to more than 64 KiB of dynamic LDS is per kernel and per device: one flag per instantiation
template <auto KERN>
void launch4(const GemvFp4Params& p, unsigned grid, size_t shmem, hipStream_t stream) {
    static RstOncePerDevice attr_once;
    if (attr_once.first()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipGetLastError();
    }
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(NT), shmem, stream, p);
}

}  // namespace

// B <= 4, K a multiple of 32 (whole scale blocks: a lane's 16-byte load is one block) and B * roundup(K, 2048) fp32 within the 128 KiB stage
int rst_gemv_mxfp4w_supported_impl(int B, int N, int K) {
    return B >= 1 && B <= 4 && N > 0 && K > 0 && K % 32 == 0 && (long)B * (((long)K + 2047) & ~2047L) <= 32768;
}

int rst_launch_gemv_mxfp4w(const GemvFp4Params& p, hipStream_t stream) {
    RST_REQUIRE(p.B >= 1 && p.B <= 4 && p.N > 0 && p.K > 0 && p.K % 32 == 0, "gemv_mxfp4w: need 1 <= B <= 4 and K %% 32 == 0 (B=%d K=%d)", p.B, p.K);
    RST_REQUIRE(p.x && p.q && p.scale && p.y, "gemv_mxfp4w: null pointer");
    RST_REQUIRE(p.prologue >= 0 && p.prologue <= 2 && (p.prologue != 1 || p.alpha), "gemv_mxfp4w: prologue must be 0 (none), 1 (RMSNorm, needs alpha) or 2 (SiLU gate)");
    RST_REQUIRE(((uintptr_t)p.q % 16) == 0 && ((uintptr_t)p.x % 16) == 0, "gemv_mxfp4w: pointers must be 16-byte aligned");
    RST_REQUIRE(!p.gate_out || (p.N % 2 == 0 && !p.res), "gemv_mxfp4w: gate_out needs an even N and no residual");
    RST_REQUIRE(p.ldx >= (p.prologue == 2 ? 2 * p.K : p.K) && p.ldy >= (p.gate_out ? p.N / 2 : p.N), "gemv_mxfp4w: ldx / ldy too small (ldx=%d ldy=%d)", p.ldx, p.ldy);
    const long KS = ((long)p.K + 2047) & ~2047L;
    const size_t lds = (size_t)p.B * KS * sizeof(float);
    RST_REQUIRE(lds <= 128 * 1024, "gemv_mxfp4w: B * roundup(K, 2048) = %ld floats do not fit the activation stage (32768)", p.B * KS);
    const bool big = (long)p.N * p.K >= (1L << 24);
    // whole rows per wave, x requested before the weight stream: batch-1 layers of K <= 4096, RMSNorm (with or without the gate) or plain.
    // (Longer plain rows -- ffn-out -- take the LDS-staged schedule below: a K-split over the waves as in lm_gemv_fp8.hip measured slower.)
    if (big && p.B == 1 && p.K <= 4096 && (p.prologue == 1 || (p.prologue == 0 && !p.gate_out))) {
        if (p.gate_out) launch4<gemv4_rows_kernel<4, true, true>>(p, cap_grid(((long)p.N / 2 + 2 * GEMV_WAVES - 1) / (2 * GEMV_WAVES), 1024), lds, stream);
        else if (p.prologue == 1) launch4<gemv4_rows_kernel<2, false, true>>(p, cap_grid(((long)p.N + 2 * GEMV_WAVES - 1) / (2 * GEMV_WAVES), 1024), lds, stream);
        else launch4<gemv4_rows_kernel<2, false, false>>(p, cap_grid(((long)p.N + 2 * GEMV_WAVES - 1) / (2 * GEMV_WAVES), 1024), lds, stream);
        return rst_check_launch("gemv_mxfp4w");
    }
    // rows per wave: 4 when that still yields >= 2 workgroups per CU, else 2 (more workgroups -> more loads in flight)
    const bool rpw4 = !p.gate_out && ((long)p.N + 15) / 16 >= 512;
    const int rows_per_group = (rpw4 ? 4 : 2) * GEMV_WAVES;
    const long groups = p.gate_out ? ((long)p.N / 2 + GEMV_WAVES - 1) / GEMV_WAVES : ((long)p.N + rows_per_group - 1) / rows_per_group;
    const unsigned grid = cap_grid(groups, lds > 48 * 1024 ? 512 : 768);
    switch (p.B * 2 + (rpw4 ? 1 : 0)) {
        case 2: launch4<gemv4_kernel<1, 2>>(p, grid, lds, stream); break;
        case 3: launch4<gemv4_kernel<1, 4>>(p, grid, lds, stream); break;
        case 4: launch4<gemv4_kernel<2, 2>>(p, grid, lds, stream); break;
        case 5: launch4<gemv4_kernel<2, 4>>(p, grid, lds, stream); break;
        case 6: launch4<gemv4_kernel<3, 2>>(p, grid, lds, stream); break;
        case 7: launch4<gemv4_kernel<3, 4>>(p, grid, lds, stream); break;
        case 8: launch4<gemv4_kernel<4, 2>>(p, grid, lds, stream); break;
        default: launch4<gemv4_kernel<4, 4>>(p, grid, lds, stream); break;
    }
    return rst_check_launch("gemv_mxfp4w");
}

int rst_launch_quant_blocks_mxfp4(const unsigned short* w, unsigned char* q, unsigned char* scale, int N, int K, hipStream_t stream) {
    RST_REQUIRE(w && q && scale && N > 0 && K > 0 && K % 32 == 0, "quant_blocks_mxfp4: bad arguments (N=%d K=%d; K must be a multiple of 32)", N, K);
    RST_REQUIRE(((uintptr_t)w % 16) == 0 && ((uintptr_t)q % 16) == 0, "quant_blocks_mxfp4: pointers must be 16-byte aligned");
    const long blocks = (long)N * (K / 32);
    hipLaunchKernelGGL(quant_blocks_mxfp4_kernel, dim3(cap_grid((blocks + NT - 1) / NT, 65536)), dim3(NT), 0, stream, w, q, scale, blocks);
    return rst_check_launch("quant_blocks_mxfp4");
}

// The schedules of the small-batch decode GEMV on quantised weights, shared by lm_gemv_fp8.hip (e4m3 bytes, one scale per row) and
// lm_gemv_fp4.hip (MXFP4: e2m1 codes, one scale byte per 32 k): y[b][n] = (res +) (bias +) sum_k P(x)[b][k] * w[n][k] with fp32
// activations and accumulation.  They mirror lm_step.hip's bf16 GEMV schedule for schedule; a lane still issues 16-byte
// non-temporal loads, which now hold more k.  Each translation unit includes this header, defines its format trait F and chooses the
// schedule per shape.  A trait supplies
//   Chunk        one lane's 16 bytes of a weight row (plus what decodes them): zero(), load(p, row, k) with row = n * F::row_stride(K)
//                and k the first k of the lane's slice, dot(x, a) = a + the slice's products in k order
//   row_stride   the distance of two rows, in the unit load() counts in (bytes / scale blocks)
//   K_PER_LOAD   k a wave covers per load (1024 / 2048); K_PER_LANE = K_PER_LOAD / 64 (16 / 32); XV = K_PER_LANE / 4
//   xs_slot      the LDS slot of element k: the stage is PERMUTED so that the j-th 16-byte read of every lane is at a lane stride of
//                16 bytes (k order would be XV reads at a lane stride of 4 * K_PER_LANE bytes: bank conflicts)
//   read_x       the XV f32x4 a lane multiplies with one Chunk, from xb = stage + chunk base + 4 * lane
//   ROW_SCALE    true: the reduced sum is multiplied by row_scales(p)[n] before bias and residual; false: dot() already applied the scale
#pragma once
#include "lm_common.h"

namespace {

constexpr int GEMV_WAVES = 4;
constexpr int NT = 64 * GEMV_WAVES;
typedef float f32x2 __attribute__((ext_vector_type(2)));

// The general schedule (gemv_kernel of lm_step.hip): activations staged once per workgroup in LDS (permuted), RPW rows per wave, the
// first weight chunk, the residual and (ROW_SCALE) the row scales of the first row group requested before the prologue, two chunks
// in flight per row in the loop.  xs holds [B][KS], KS = K rounded up to K_PER_LOAD; slots beyond K are never read.
template <class F, int B, int RPW>
__global__ __launch_bounds__(NT) void gemvq_kernel(const GemvQuantParams p) {
    using Chunk = typename F::Chunk;
    constexpr int KPL = F::K_PER_LOAD;
    extern __shared__ __attribute__((aligned(16))) float xs[];
    __shared__ float red[GEMV_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.K, KS = (K + KPL - 1) & ~(KPL - 1), RS = F::row_stride(K);
    const int half = p.N / 2;
    const int groups = p.gate_out ? (half + GEMV_WAVES - 1) / GEMV_WAVES : (p.N + RPW * GEMV_WAVES - 1) / (RPW * GEMV_WAVES);
    // gate_out (RPW == 2): the wave's two rows are (n, N/2 + n) = (u_n, v_n) of a stacked gated layer, one output silu(u) * v
    auto row_of = [&](int grp, int r) {
        const int n = grp * GEMV_WAVES + wave;
        return p.gate_out ? r * half + min(n, half - 1) : min(n * RPW + r, p.N - 1);
    };
    Chunk wpre[RPW];
    float spre[RPW], rpre[RPW][B];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        wpre[r].zero();
        if (blockIdx.x < groups && lane * F::K_PER_LANE < K) wpre[r].load(p, (long)row_of(blockIdx.x, r) * RS, lane * F::K_PER_LANE);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        if constexpr (F::ROW_SCALE) spre[r] = lane == 0 && blockIdx.x < groups ? F::row_scales(p)[row_of(blockIdx.x, r)] : 0.f;
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
                if (k < K) xs[b * KS + F::xs_slot(k)] = xr[i] * (p.alpha[k] * r);
            }
            for (int k = tid + XR * NT; k < K; k += NT) xs[b * KS + F::xs_slot(k)] = p.x[(long)b * p.ldx + k] * (p.alpha[k] * r);
        }
    } else if (p.prologue == 2) {    // SiLU gate: x holds [B][2K] = [u ; v], xs = silu(u) * v   (modules/gating.py:12-22)
        for (int b = 0; b < B; ++b)
            for (int k = tid; k < K; k += NT) xs[b * KS + F::xs_slot(k)] = silu(p.x[(long)b * p.ldx + k]) * p.x[(long)b * p.ldx + K + k];
    } else {
        for (int b = 0; b < B; ++b)
            for (int k = tid; k < K; k += NT) xs[b * KS + F::xs_slot(k)] = p.x[(long)b * p.ldx + k];
    }
    __syncthreads();

    // ---- row groups, grid-strided: RPW rows per wave, 16 bytes per lane per row per iteration, two iterations in flight
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int n0 = (grp * GEMV_WAVES + wave) * RPW;
        float acc[RPW][B];
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int b = 0; b < B; ++b) acc[r][b] = 0.f;
        long wrow[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) wrow[r] = (long)row_of(grp, r) * RS;
        auto fma = [&](const Chunk (&wv)[RPW], int k) {          // k = c * K_PER_LOAD + K_PER_LANE * lane
#pragma unroll
            for (int b = 0; b < B; ++b) {
                f32x4 x[F::XV];
                F::read_x(xs + b * KS + (k & ~(KPL - 1)) + lane * 4, x);
#pragma unroll
                for (int r = 0; r < RPW; ++r) acc[r][b] = wv[r].dot(x, acc[r][b]);
            }
        };
        const bool first = grp == (int)blockIdx.x;
        int k = lane * F::K_PER_LANE;
        if (first && k < K) {        // the prefetched chunk
            fma(wpre, k);
            k += KPL;
        }
        for (; k + KPL < K; k += 2 * KPL) {
            Chunk wa[RPW], wb[RPW];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                wa[r].load(p, wrow[r], k);
                wb[r].load(p, wrow[r], k + KPL);
            }
            fma(wa, k);
            fma(wb, k + KPL);
        }
        if (k < K) {
            Chunk wa[RPW];
#pragma unroll
            for (int r = 0; r < RPW; ++r) wa[r].load(p, wrow[r], k);
            fma(wa, k);
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int b = 0; b < B; ++b) acc[r][b] = wave_sum(acc[r][b]);
        if (lane != 0) continue;
        float sc[RPW];
        if constexpr (F::ROW_SCALE) {
#pragma unroll
            for (int r = 0; r < RPW; ++r) sc[r] = first ? spre[r] : F::row_scales(p)[row_of(grp, r)];
        }
        auto sum = [&](int r, int b) {   // the row's dot product
            if constexpr (F::ROW_SCALE) return acc[r][b] * sc[r];
            else return acc[r][b];
        };
        if (p.gate_out) {
            const int n = grp * GEMV_WAVES + wave;
            if (n < half)
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    float u = sum(0, b), v = sum(RPW - 1, b);
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
                    float sb = sum(r, b);
                    if (p.bias) sb += p.bias[n];
                    p.y[o] = p.res ? (first ? rpre[r][b] : p.res[o]) + sb : sb;
                }
            }
    }
}

// Batch-1 whole rows per wave for K <= 4096 (gemv_norm_kernel of lm_step.hip): x (and alpha) are requested FIRST, then every weight
// byte (and scale) of the wave's rows, and the norm runs on data that arrives ahead of the weights.  NORM = false: the same schedule
// on a plain vector.  A K <= 4096 row is at most PRE = 4096 / K_PER_LOAD loads per lane (8 for bf16), so PRE * RPW loads x 16 bytes
// per lane are in flight; each launcher picks RPW.  GATE: the wave's rows are PPW = RPW / 2 (u, v) pairs
// (n, N/2 + n), (n + 1, N/2 + n + 1), ...
template <class F, int RPW, bool GATE, bool NORM>
__global__ __launch_bounds__(NT) void gemvq_rows_kernel(const GemvQuantParams p) {
    using Chunk = typename F::Chunk;
    constexpr int KPL = F::K_PER_LOAD, PRE = 4096 / KPL, XR = 16, PPW = RPW / 2;
    extern __shared__ __attribute__((aligned(16))) float xs[];   // [KS] permuted
    __shared__ float red[GEMV_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.K, RS = F::row_stride(K), half = p.N / 2;
    const int groups = GATE ? (half + PPW * GEMV_WAVES - 1) / (PPW * GEMV_WAVES) : (p.N + RPW * GEMV_WAVES - 1) / (RPW * GEMV_WAVES);
    const int kl = lane * F::K_PER_LANE;

    float xa[XR], al[XR];            // K <= XR * NT = 4096 (launch check)
#pragma unroll
    for (int i = 0; i < XR; ++i) {
        const int k = tid + i * NT;
        xa[i] = k < K ? p.x[k] : 0.f;
        al[i] = NORM && k < K ? p.alpha[k] : 0.f;
    }
    Chunk buf[PRE][RPW];
    float sc[RPW];
    auto row_of = [&](int grp, int r) {
        const int n = grp * GEMV_WAVES + wave;
        return GATE ? (r & 1) * half + min(PPW * n + (r >> 1), half - 1) : min(n * RPW + r, p.N - 1);
    };
    auto issue = [&](int grp) {      // all chunks of the wave's rows, then (ROW_SCALE) their scales
#pragma unroll
        for (int j = 0; j < PRE; ++j)
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int kk = j * KPL + kl;
                if (kk < K) buf[j][r].load(p, (long)row_of(grp, r) * RS, kk);
                else buf[j][r].zero();
            }
        if constexpr (F::ROW_SCALE) {
#pragma unroll
            for (int r = 0; r < RPW; ++r) sc[r] = F::row_scales(p)[row_of(grp, r)];
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
        if (k < K) xs[F::xs_slot(k)] = xa[i];
    }
    __syncthreads();

    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        if (grp != (int)blockIdx.x) issue(grp);
        float acc[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) acc[r] = 0.f;
#pragma unroll
        for (int j = 0; j < PRE; ++j) {
            if (j * KPL + kl < K) {
                f32x4 x[F::XV];
                F::read_x(xs + j * KPL + lane * 4, x);
#pragma unroll
                for (int r = 0; r < RPW; ++r) acc[r] = buf[j][r].dot(x, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r) acc[r] = wave_sum_fast(acc[r]);
        if (lane != 0) continue;
        auto sum = [&](int r) {          // the row's dot product
            if constexpr (F::ROW_SCALE) return acc[r] * sc[r];
            else return acc[r];
        };
        const int n = grp * GEMV_WAVES + wave;
        if (GATE) {
#pragma unroll
            for (int h = 0; h < PPW; ++h) {
                const int o = PPW * n + h;
                if (o < half) {
                    float u = sum(2 * h), v = sum(2 * h + 1);
                    if (p.bias) { u += p.bias[o]; v += p.bias[half + o]; }
                    p.y[o] = silu(u) * v;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int o = n * RPW + r;
                if (o < p.N) {
                    float sb = sum(r);
                    if (p.bias) sb += p.bias[o];
                    p.y[o] = p.res ? p.res[o] + sb : sb;
                }
            }
        }
    }
}

template <auto KERN>
void launch_gemvq(const GemvQuantParams& p, unsigned grid, size_t shmem, hipStream_t stream) {
    rst_allow_dynamic_lds<KERN>(128 * 1024);
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(NT), shmem, stream, p);
}

// B <= 4, K a multiple of kmult (a lane's 16-byte load must not straddle a row or a scale block) and B * roundup(K, K_PER_LOAD) fp32
// within the 128 KiB stage
template <class F>
int gemvq_supported(int B, int N, int K, int kmult) {
    return B >= 1 && B <= 4 && N > 0 && K > 0 && K % kmult == 0 && (long)B * (((long)K + F::K_PER_LOAD - 1) & ~(long)(F::K_PER_LOAD - 1)) <= 32768;
}

// the argument checks of both launchers; *lds = the bytes of the activation stage
template <class F>
int gemvq_check(const GemvQuantParams& p, const char* op, int kmult, size_t* lds) {
    RST_REQUIRE(p.B >= 1 && p.B <= 4 && p.N > 0 && p.K > 0 && p.K % kmult == 0, "%s: need 1 <= B <= 4 and K %% %d == 0 (B=%d K=%d)", op, kmult, p.B, p.K);
    RST_REQUIRE(p.x && p.q && p.scale && p.y, "%s: null pointer", op);
    RST_REQUIRE(p.prologue >= 0 && p.prologue <= 2 && (p.prologue != 1 || p.alpha), "%s: prologue must be 0 (none), 1 (RMSNorm, needs alpha) or 2 (SiLU gate)", op);
    RST_REQUIRE(((uintptr_t)p.q % 16) == 0 && ((uintptr_t)p.x % 16) == 0, "%s: pointers must be 16-byte aligned", op);
    RST_REQUIRE(!p.gate_out || (p.N % 2 == 0 && !p.res), "%s: gate_out needs an even N and no residual", op);
    RST_REQUIRE(p.ldx >= (p.prologue == 2 ? 2 * p.K : p.K) && p.ldy >= (p.gate_out ? p.N / 2 : p.N), "%s: ldx / ldy too small (ldx=%d ldy=%d)", op, p.ldx, p.ldy);
    const long KS = ((long)p.K + F::K_PER_LOAD - 1) & ~(long)(F::K_PER_LOAD - 1);
    *lds = (size_t)p.B * KS * sizeof(float);
    RST_REQUIRE(*lds <= 128 * 1024, "%s: B * roundup(K, %d) = %ld floats do not fit the activation stage (32768)", op, F::K_PER_LOAD, p.B * KS);
    return RST_OK;
}

// the general schedule's instance for (B, rows per wave)
template <class F>
void launch_gemvq_general(const GemvQuantParams& p, bool rpw4, unsigned grid, size_t lds, hipStream_t stream) {
    switch (p.B * 2 + (rpw4 ? 1 : 0)) {
        case 2: launch_gemvq<gemvq_kernel<F, 1, 2>>(p, grid, lds, stream); break;
        case 3: launch_gemvq<gemvq_kernel<F, 1, 4>>(p, grid, lds, stream); break;
        case 4: launch_gemvq<gemvq_kernel<F, 2, 2>>(p, grid, lds, stream); break;
        case 5: launch_gemvq<gemvq_kernel<F, 2, 4>>(p, grid, lds, stream); break;
        case 6: launch_gemvq<gemvq_kernel<F, 3, 2>>(p, grid, lds, stream); break;
        case 7: launch_gemvq<gemvq_kernel<F, 3, 4>>(p, grid, lds, stream); break;
        case 8: launch_gemvq<gemvq_kernel<F, 4, 2>>(p, grid, lds, stream); break;
        default: launch_gemvq<gemvq_kernel<F, 4, 4>>(p, grid, lds, stream); break;
    }
}

}  // namespace

// Per-row LoRA adapters from a device-resident bank: the two thin products behind an adapted LM linear, every row of the call with the
// adapter its stream selected (GPT.load_adapter_bank / set_adapter_ids).
//
//   shrink:  a[row][0:r]  = post_scale * A_bank[id(row)] . P(x[row])        A_bank bf16 [n_adapters][r][K], x fp32, P = none / RMSNorm / SiLU gate
//   expand:  y[row][0:N] += B_bank[id(row)] . a[row]                        B_bank bf16 [n_adapters][N][r], in place on the base product
//   id(row) = ids[row / rows_per_id]; a row whose id fails `(unsigned)id < n_adapters` is a base-model row: shrink writes zeros, expand
//   leaves y[row] alone, and neither reads the bank.
//
// Both launches are bound by memory and launch latency (r <= 256: a few hundred KB per row at most), so there are no matrix
// instructions here.  What they promise instead is ONE summation schedule per output element that depends on (K, r, N) only -- never on
// the row index, the number of rows, the id or what other rows hold -- and no floating-point atomics: a row's result is bit-identical
// whatever batch it sits in.
//
// Shrink = the schedule of gemv_kernel (lm_step.hip) with one activation row per workgroup: workgroup (row, slab of LB_SLAB adapter
// rows), P(x[row]) staged once in LDS, a wave owns two adapter rows, a lane multiplies 8 consecutive k (one 16-byte load) of every
// 512-wide chunk into ONE fmaf chain per adapter row, ascending k; the 64 lanes meet in the xor butterfly; post_scale multiplies the sum.
// Expand: one thread per output, ONE fmaf chain over j = 0 .. r-1 started at zero (a[row] read from LDS), then one addition into y.
#include "lm_common.h"

namespace {

constexpr int LB_WAVES = 4;
constexpr int LB_RPW = 2;                      // adapter rows per wave
constexpr int LB_SLAB = LB_WAVES * LB_RPW;     // adapter rows per workgroup (r % 16 == 0: slabs are always full)
constexpr int LB_THREADS = 64 * LB_WAVES;

// (the fmaf chain of 8 k: bf16_dot8, lm_common.h)
__device__ __forceinline__ u32x4 load8(const unsigned short* w) { return *reinterpret_cast<const u32x4*>(w); }

__global__ __launch_bounds__(LB_THREADS) void lora_bank_shrink_kernel(const LoraBankShrinkParams p) {
    extern __shared__ __attribute__((aligned(16))) float xs[];   // [K] staged activation, then [LB_WAVES] reduction scratch (K % 8 == 0)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = p.K;
    float* red = xs + K;
    const int slabs = p.r / LB_SLAB;
    const long row = blockIdx.x / slabs;
    const int j0 = ((int)(blockIdx.x - row * slabs)) * LB_SLAB + wave * LB_RPW;
    float* out = p.a + row * p.r + j0;
    const int id = p.ids[row / p.rows_per_id];
    if ((unsigned)id >= (unsigned)p.n_adapters) {      // base-model row (uniform over the workgroup: in front of every barrier)
        if (lane < LB_RPW) out[lane] = 0.f;
        return;
    }
    // the first weight chunk is requested before the activation prologue, as in gemv_kernel: the two load chains overlap
    const unsigned short* w0 = p.A + ((long)id * p.r + j0) * K;
    const unsigned short* w1 = w0 + K;
    int k = lane * 8;
    u32x4 pre0 = u32x4{0u, 0u, 0u, 0u}, pre1 = pre0;
    if (k < K) { pre0 = load8(w0 + k); pre1 = load8(w1 + k); }

    const float* x = p.x + row * p.ldx;
    if (p.prologue == 1) {           // RMSNorm: x * alpha * rsqrt(eps + mean(x^2)), the arithmetic of gemv_kernel's prologue 1
        float s = 0.f;
        for (int i = tid; i < K; i += LB_THREADS) { const float v = x[i]; s = fmaf(v, v, s); }
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < LB_WAVES; ++w) tot += red[w];
        const float rs = 1.0f / sqrtf(p.eps + tot / (float)K);
        for (int i = tid; i < K; i += LB_THREADS) xs[i] = x[i] * (p.alpha[i] * rs);
    } else if (p.prologue == 2) {    // SiLU gate: x holds [u | v], 2K wide
        for (int i = tid; i < K; i += LB_THREADS) xs[i] = silu(x[i]) * x[K + i];
    } else {
        for (int i = tid; i < K; i += LB_THREADS) xs[i] = x[i];
    }
    __syncthreads();

    float acc0 = 0.f, acc1 = 0.f;
    auto fma8 = [&](const u32x4& a0, const u32x4& a1, int at) {
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(xs + at);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(xs + at + 4);
        acc0 = bf16_dot8(a0, x0, x1, acc0);
        acc1 = bf16_dot8(a1, x0, x1, acc1);
    };
    if (k < K) {
        fma8(pre0, pre1, k);
        k += 512;
    }
    for (; k + 512 < K; k += 1024) {     // two chunks of both rows in flight
        const u32x4 a0 = load8(w0 + k), a1 = load8(w1 + k), b0 = load8(w0 + k + 512), b1 = load8(w1 + k + 512);
        fma8(a0, a1, k);
        fma8(b0, b1, k + 512);
    }
    if (k < K) {
        const u32x4 a0 = load8(w0 + k), a1 = load8(w1 + k);
        fma8(a0, a1, k);
    }
    acc0 = wave_sum(acc0);
    acc1 = wave_sum(acc1);
    if (lane == 0) {
        out[0] = acc0 * p.post_scale;
        out[1] = acc1 * p.post_scale;
    }
}

__global__ __launch_bounds__(LB_THREADS) void lora_bank_expand_kernel(const LoraBankExpandParams p) {
    __shared__ __attribute__((aligned(16))) float as[256];       // a[row] (r <= 256)
    const int tid = threadIdx.x, r = p.r;
    const long row = blockIdx.x / p.nblk;
    const long n = (long)(blockIdx.x - row * p.nblk) * LB_THREADS + tid;
    const int id = p.ids[row / p.rows_per_id];
    if ((unsigned)id >= (unsigned)p.n_adapters) return;          // base-model row: y[row] keeps its bits
    if (tid < r) as[tid] = p.a[row * r + tid];
    __syncthreads();
    if (n >= p.N) return;
    const unsigned short* w = p.B + ((long)id * p.N + n) * r;
    float acc = 0.f;
    for (int j = 0; j < r; j += 16) {
        const u32x4 b0 = load8(w + j), b1 = load8(w + j + 8);
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(as + j), a1 = *reinterpret_cast<const f32x4*>(as + j + 4);
        const f32x4 a2 = *reinterpret_cast<const f32x4*>(as + j + 8), a3 = *reinterpret_cast<const f32x4*>(as + j + 12);
        acc = bf16_dot8(b0, a0, a1, acc);
        acc = bf16_dot8(b1, a2, a3, acc);
    }
    float* y = p.y + row * p.ldy + n;
    *y = *y + acc;
}

int check_common(const char* what, const void* bank, const int* ids, int rows, int rows_per_id, int n_ids, int n_adapters) {
    RST_REQUIRE(bank && ids, "%s: null pointer", what);
    RST_REQUIRE(((uintptr_t)bank % 16) == 0, "%s: the bank must be 16-byte aligned", what);
    RST_REQUIRE(rows >= 1 && rows_per_id >= 1 && rows % rows_per_id == 0 && n_ids == rows / rows_per_id,
                "%s: rows (%d) must be n_ids (%d) groups of rows_per_id (%d)", what, rows, n_ids, rows_per_id);
    RST_REQUIRE(n_adapters >= 1, "%s: n_adapters (%d) must be >= 1", what, n_adapters);
    return RST_OK;
}

}  // namespace

int rst_lora_bank_supported_impl(int K, int r, int N) {
    return K >= 8 && K % 8 == 0 && K <= 16384 && r >= 16 && r % 16 == 0 && r <= 256 && N >= 1;
}

int rst_launch_lora_bank_shrink(const LoraBankShrinkParams& p, int n_ids, hipStream_t stream) {
    RST_REQUIRE(rst_lora_bank_supported_impl(p.K, p.r, 1), "lora_bank_shrink: need K %% 8 == 0, K <= 16384, r %% 16 == 0, r <= 256 (K=%d r=%d)", p.K, p.r);
    if (const int rc = check_common("lora_bank_shrink", p.A, p.ids, (int)p.rows, p.rows_per_id, n_ids, p.n_adapters)) return rc;
    RST_REQUIRE(p.x && p.a, "lora_bank_shrink: null pointer");
    RST_REQUIRE(p.prologue >= 0 && p.prologue <= 2, "lora_bank_shrink: prologue must be 0 (none), 1 (RMSNorm) or 2 (SiLU gate)");
    RST_REQUIRE(p.prologue != 1 || p.alpha, "lora_bank_shrink: the RMSNorm prologue needs alpha");
    RST_REQUIRE(p.ldx >= (p.prologue == 2 ? 2 * p.K : p.K), "lora_bank_shrink: ldx (%d) below the row width (K=%d, prologue %d)", p.ldx, p.K, p.prologue);
    const long grid = p.rows * (p.r / LB_SLAB);
    RST_REQUIRE(grid <= 0x7fffffffL, "lora_bank_shrink: rows * r / %d = %ld workgroups exceed one grid", LB_SLAB, grid);
    const size_t lds = (size_t)(p.K + LB_WAVES) * sizeof(float);
    rst_allow_dynamic_lds<lora_bank_shrink_kernel>(128 * 1024);      // K = 16384 stages 64 KiB and the reduction scratch behind it
    hipLaunchKernelGGL(lora_bank_shrink_kernel, dim3((unsigned)grid), dim3(LB_THREADS), lds, stream, p);
    return rst_check_launch("lora_bank_shrink");
}

int rst_launch_lora_bank_expand(LoraBankExpandParams p, int n_ids, hipStream_t stream) {
    RST_REQUIRE(rst_lora_bank_supported_impl(8, p.r, p.N), "lora_bank_expand: need r %% 16 == 0, r <= 256 and N >= 1 (r=%d N=%d)", p.r, p.N);
    if (const int rc = check_common("lora_bank_expand", p.B, p.ids, (int)p.rows, p.rows_per_id, n_ids, p.n_adapters)) return rc;
    RST_REQUIRE(p.a && p.y, "lora_bank_expand: null pointer");
    RST_REQUIRE(p.ldy >= p.N, "lora_bank_expand: ldy (%d) < N (%d)", p.ldy, p.N);
    p.nblk = (p.N + LB_THREADS - 1) / LB_THREADS;
    const long grid = p.rows * p.nblk;
    RST_REQUIRE(grid <= 0x7fffffffL, "lora_bank_expand: rows * ceil(N / %d) = %ld workgroups exceed one grid", LB_THREADS, grid);
    hipLaunchKernelGGL(lora_bank_expand_kernel, dim3((unsigned)grid), dim3(LB_THREADS), 0, stream, p);
    return rst_check_launch("lora_bank_expand");
}

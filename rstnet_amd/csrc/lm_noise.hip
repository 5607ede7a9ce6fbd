// Exp(1) noise of the samplers as a counter-based stream: noise[b][c] is a pure function of (seed[b], the frame
// counter of stream b, c), so a conversation's draws do not depend on its row, on the batch around it or on what the process drew
// before.  Philox4x32-10 (Salmon et al., SC'11; the standard multipliers and key increments): key = the seed's two halves, counter =
// (c >> 2, 0, lo32(frame), hi32(frame)), word c & 3.  x -> u = ((x >> 9) + 0.5) * 2^-23 is exact in fp32 (a 23-bit integer plus a
// half) and lies in [2^-24, 1 - 2^-24]; noise = -logf(u) is finite and > 0 (at most 24 ln 2 = 16.64).  The seeds and the counters
// are read from device memory: one captured launch serves counters that advance (lm_ring_commit) and reset (reset_streams).
#include "lm_common.h"

namespace {

struct Philox4 { unsigned x, y, z, w; };

__device__ __forceinline__ Philox4 philox4x32_10(Philox4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c.x, p1 = 0xCD9E8D57ull * c.z;
        c = Philox4{(unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

__device__ __forceinline__ float exp1_of(unsigned x) { return -logf(((float)(x >> 9) + 0.5f) * 0x1p-23f); }

// one thread = one counter = columns 4q .. 4q + 3 of row blockIdx.y; columns >= n_cols are not written
__global__ __launch_bounds__(256) void noise_exp_kernel(const LmNoiseParams p) {
    const int q = blockIdx.x * 256 + threadIdx.x, c0 = q * 4;
    if (c0 >= p.n_cols) return;
    const long b = blockIdx.y;
    const unsigned long long seed = p.seed_dev[b];
    const unsigned long long f = (unsigned long long)p.frame_dev[b * p.frame_stride];
    const Philox4 r = philox4x32_10(Philox4{(unsigned)q, 0u, (unsigned)f, (unsigned)(f >> 32)}, (unsigned)seed, (unsigned)(seed >> 32));
    const float v[4] = {exp1_of(r.x), exp1_of(r.y), exp1_of(r.z), exp1_of(r.w)};
    float* row = p.noise + b * p.noise_stride + c0;
    const int n = min(4, p.n_cols - c0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) row[i] = v[i];
}

}  // namespace

int rst_launch_lm_noise(const LmNoiseParams& p, hipStream_t stream) {
    RST_REQUIRE(p.noise && p.seed_dev && p.frame_dev, "noise_exp: null pointer");
    RST_REQUIRE(p.B >= 1 && p.n_cols >= 1, "noise_exp: bad sizes (B=%d n_cols=%d)", p.B, p.n_cols);
    RST_REQUIRE(p.noise_stride >= p.n_cols, "noise_exp: row stride %d < n_cols %d", p.noise_stride, p.n_cols);
    RST_REQUIRE(p.frame_stride >= 0, "noise_exp: counter stride %d (0: one for the batch, n: stream b reads frame_dev[b * n])", p.frame_stride);
    RST_REQUIRE(p.B <= 65535, "noise_exp: %d rows exceed the grid", p.B);
    const int counters = (p.n_cols + 3) / 4;
    hipLaunchKernelGGL(noise_exp_kernel, dim3((counters + 255) / 256, p.B), dim3(256), 0, stream, p);
    return rst_check_launch("noise_exp");
}

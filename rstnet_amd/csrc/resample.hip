// Polyphase sinc sample-rate conversion of a ragged batch in ONE launch (rst_resample_sinc, include/rstnet_hip.h): whole signals in
// front of the codec (codec/audio_resample.py: resample_device) and, with lead = 0 over a history + chunk buffer, one frame of a live
// stream (StreamResampler).  A workgroup owns RESAMPLE_TILE consecutive outputs of one row, one output per lane: the input slab the tile
// reads goes to LDS once (s16 converted there), the tap table stays in global memory (54 .. 201 KB for the audio rates: L2-resident, and
// stored tap-major so that the lanes of a wave, whose phases are consecutive, read consecutive floats).
//
// Every output is the same chain whatever tile, row, chunk or staging route it falls in: acc = 0; for k = 0 .. L-1 in this order
// acc = fmaf(filt[k][p], X[j * o + k - lead], acc) -- one fp32 accumulator, always FMA, never re-associated.  The streamed and the
// whole-signal conversions are bit-identical because of it.
#include "rst_common.h"
#include "rst_kernels.h"

namespace {

constexpr int TILE = RST_RESAMPLE_TILE;         // outputs per workgroup = threads per workgroup
constexpr int SLAB_MAX_BYTES = 32 * 1024;       // larger input spans per tile (orig / new above ~ 30) are read from global instead

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<short>(short v) { return (float)v * 3.0517578125e-05f; }   // 2^-15, exact

// X_b[t]: the row's sample inside [0, len), zero outside
template <typename T> __device__ __forceinline__ float sample(const T* __restrict__ xr, long t, int len) {
    return t >= 0 && t < (long)len ? to_f32<T>(xr[t]) : 0.f;
}

template <typename T, bool STAGED>
__global__ __launch_bounds__(TILE) void resample_sinc_kernel(const T* __restrict__ x, long x_row_stride, int T_in,
                                                             const int* __restrict__ in_lengths, const float* __restrict__ filt,
                                                             int o, int n, int L, int lead, float* __restrict__ y, long y_row_stride,
                                                             const int* __restrict__ out_lengths, int T_out, int tiles) {
    extern __shared__ __attribute__((aligned(16))) float slab[];
    const int b = (int)(blockIdx.x / (unsigned)tiles);
    const int i0 = (int)(blockIdx.x % (unsigned)tiles) * TILE;
    const int i = i0 + (int)threadIdx.x;
    int valid = out_lengths ? out_lengths[b] : T_out;
    valid = min(max(valid, 0), T_out);
    float* yr = y + (long)b * y_row_stride;
    if (i0 >= valid) {                       // a tile of the zero tail (uniform: no barrier is skipped by part of a workgroup)
        if (i < T_out) yr[i] = 0.f;
        return;
    }
    int len = in_lengths ? in_lengths[b] : T_in;
    len = min(max(len, 0), T_in);
    const T* xr = x + (long)b * x_row_stride;
    const int j0 = i0 / n;
    const long base = (long)j0 * o - lead;   // first input index the tile reads
    if (STAGED) {
        const int j1 = (min(i0 + TILE, valid) - 1) / n;
        const int span = (j1 - j0) * o + L;  // <= the launch's slab size: j1 - j0 <= (TILE + n - 2) / n
        for (int s = (int)threadIdx.x; s < span; s += TILE) slab[s] = sample<T>(xr, base + s, len);
        __syncthreads();
    }
    if (i >= T_out) return;
    float acc = 0.f;
    if (i < valid) {
        const int j = i / n, p = i - j * n;
        const int off = (j - j0) * o;
        if (filt) {
            const float* f = filt + p;
#pragma unroll 4
            for (int k = 0; k < L; ++k) {        // (unrolled for loads in flight; the chain itself stays in tap order)
                const float xv = STAGED ? slab[off + k] : sample<T>(xr, base + off + k, len);
                acc = fmaf(f[(long)k * n], xv, acc);
            }
        } else {                             // o = n = L = 1: the conversion alone
            acc = STAGED ? slab[off] : sample<T>(xr, base + off, len);
        }
    }
    yr[i] = acc;
}

// floats of input a tile can read: j spans at most (TILE + n - 2) / n input strides, plus the taps
inline long slab_floats(int o, int n, int L) { return (long)((TILE + n - 2) / n) * o + L; }

template <typename T>
int launch(const T* x, long x_row_stride, int T_in, const int* in_lengths, const float* filt, int o, int n, int L, int lead, float* y,
           long y_row_stride, const int* out_lengths, int B, int T_out, hipStream_t stream) {
    const int tiles = (T_out + TILE - 1) / TILE;
    const long span = slab_floats(o, n, L);
    const dim3 grid((unsigned)((long)tiles * B));
    if (span * (long)sizeof(float) <= SLAB_MAX_BYTES)
        hipLaunchKernelGGL((resample_sinc_kernel<T, true>), grid, dim3(TILE), (size_t)span * sizeof(float), stream, x, x_row_stride, T_in,
                           in_lengths, filt, o, n, L, lead, y, y_row_stride, out_lengths, T_out, tiles);
    else
        hipLaunchKernelGGL((resample_sinc_kernel<T, false>), grid, dim3(TILE), 0, stream, x, x_row_stride, T_in, in_lengths, filt, o, n,
                           L, lead, y, y_row_stride, out_lengths, T_out, tiles);
    return rst_check_launch("resample_sinc");
}

}  // namespace

int rst_resample_slab_bytes(int o, int n, int L) {
    const long bytes = slab_floats(o, n, L) * (long)sizeof(float);
    return bytes <= SLAB_MAX_BYTES ? (int)bytes : 0;
}

int rst_launch_resample_sinc(const void* x, int x_dtype, long x_row_stride, int T_in, const int* in_lengths, const float* filt, int o,
                             int n, int L, int lead, float* y, long y_row_stride, const int* out_lengths, int B, int T_out,
                             hipStream_t stream) {
    RST_REQUIRE(o >= 1 && n >= 1 && L >= 1 && lead >= 0, "resample_sinc: o, n, L >= 1 and lead >= 0 required (o=%d n=%d L=%d lead=%d)", o, n, L, lead);
    RST_REQUIRE(x_dtype == 0 || x_dtype == 1, "resample_sinc: x_dtype %d (0 = f32, 1 = s16)", x_dtype);
    RST_REQUIRE(B >= 0 && T_out >= 0 && T_in >= 0, "resample_sinc: negative size (B=%d T_in=%d T_out=%d)", B, T_in, T_out);
    RST_REQUIRE(x_row_stride >= T_in && y_row_stride >= T_out, "resample_sinc: a row stride is shorter than its row");
    RST_REQUIRE(y || B == 0 || T_out == 0, "resample_sinc: null output");
    RST_REQUIRE(x || T_in == 0, "resample_sinc: null input");
    RST_REQUIRE(filt || (o == 1 && n == 1 && L == 1), "resample_sinc: null filter table (allowed at o = n = L = 1 only)");
    if (B == 0 || T_out == 0) return RST_OK;
    // the last input index a row can be asked for, and the grid, stay inside 31 bits
    RST_REQUIRE(T_out <= 0x7fffffff - TILE && ((long)(T_out - 1) / n) * o + L < 0x7fffffffL, "resample_sinc: sample index beyond 2^31");
    RST_REQUIRE((long)((T_out + TILE - 1) / TILE) * B < 0x7fffffffL, "resample_sinc: too many tiles (B=%d T_out=%d)", B, T_out);
    if (x_dtype == 1)
        return launch<short>((const short*)x, x_row_stride, T_in, in_lengths, filt, o, n, L, lead, y, y_row_stride, out_lengths, B,
                             T_out, stream);
    return launch<float>((const float*)x, x_row_stride, T_in, in_lengths, filt, o, n, L, lead, y, y_row_stride, out_lengths, B, T_out,
                         stream);
}

// Packed frame ingress and egress (rst_frame_ingress / rst_frame_egress, include/rstnet_hip.h): the two ends of a served frame.  One
// record per row of the batch, REC bytes apart (a multiple of 16), a 16-byte header and then the frame's samples in the row's own
// transport (fmt[b]: -1 free row, 0 f32, 1 s16).  The ingress turns the uploaded records into the codec's fp32 [B][1][F] input, the
// egress turns the decoder's fp32 output, the frame's text token and the per-stream frame counter into the records one download
// carries back -- validity, zero fill of rows inside their delay and the s16 encoding included, so the host builds no row list.
//
// Both are HBM-bound copies.  A record's payload starts 16 bytes into a 16-byte-aligned record, so the record side always moves 16
// bytes per lane (8 for four s16 samples on the way in); the fp32 side is a dense [B][F] array whose row b starts at b * F floats: it
// moves float4 where that is a multiple of four and the array itself starts on a 16-byte boundary (uniform per workgroup), plain dwords
// otherwise and in the tail.  No LDS.
#include "rst_common.h"
#include "rst_kernels.h"

namespace {

constexpr int FIO_THREADS = 256;

__device__ __forceinline__ int fio_fmt(const int* __restrict__ fmt, int b) { return fmt[b]; }

// (int16)(clamp(x, -1, 1) * 32767.0f), truncated toward zero: one rounded multiply, nothing to contract it with; NaN -> 0
__device__ __forceinline__ unsigned fio_s16(float x) {
    if (!(x == x)) return 0u;
    const float c = fminf(fmaxf(x, -1.0f), 1.0f);
    return (unsigned)((int)__fmul_rn(c, 32767.0f)) & 0xffffu;
}

__device__ __forceinline__ float fio_from_s16(unsigned bits16) { return (float)(short)bits16 * 3.0517578125e-05f; }   // 2^-15: exact

// one lane: four consecutive samples of one row
__global__ __launch_bounds__(FIO_THREADS) void frame_ingress_kernel(const unsigned char* __restrict__ staged, const int* __restrict__ fmt,
                                                                    float* __restrict__ pcm, int F, long rec_stride, int wide) {
    const int b = (int)blockIdx.y;
    const int q = (int)(blockIdx.x * FIO_THREADS + threadIdx.x);
    const int i0 = q * 4;
    if (i0 >= F) return;
    const unsigned char* rec = staged + (long)b * rec_stride;
    const int f = fio_fmt(fmt, b);
    const int present = *reinterpret_cast<const int*>(rec);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (present != 0 && f >= 0) {
        if (f == 1) {                                        // 8 aligned bytes: 16 + 8 q
            const uint2 w = *reinterpret_cast<const uint2*>(rec + 16 + (long)q * 8);
            v[0] = fio_from_s16(w.x & 0xffffu); v[1] = fio_from_s16(w.x >> 16);
            v[2] = fio_from_s16(w.y & 0xffffu); v[3] = fio_from_s16(w.y >> 16);
        } else {                                             // 16 aligned bytes: 16 + 16 q (the record is padded to it)
            const uint4 w = *reinterpret_cast<const uint4*>(rec + 16 + (long)q * 16);
            v[0] = __uint_as_float(w.x); v[1] = __uint_as_float(w.y); v[2] = __uint_as_float(w.z); v[3] = __uint_as_float(w.w);
        }
    }
    const long row = (long)b * F;
    float* out = pcm + row + i0;
    if (i0 + 3 < F && wide && ((row & 3) == 0)) {
        *reinterpret_cast<float4*>(out) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < F) out[j] = v[j];
    }
}

__device__ __forceinline__ float fio_load(const float* __restrict__ w, int i, int F) { return i < F ? w[i] : 0.f; }

// one lane: one 16-byte chunk of one record; chunk 0 is the header, chunk c >= 1 the payload bytes [16 (c - 1), 16 c)
__global__ __launch_bounds__(FIO_THREADS) void frame_egress_kernel(const float* __restrict__ wav, const long* __restrict__ tokens,
                                                                   int tok_stride, const long* __restrict__ offset_dev, int max_delay,
                                                                   const int* __restrict__ fmt, unsigned char* __restrict__ out, int F,
                                                                   long rec_stride, int wide) {
    const int b = (int)blockIdx.y;
    const int c = (int)(blockIdx.x * FIO_THREADS + threadIdx.x);
    const int chunks = (int)(rec_stride >> 4);
    if (c >= chunks) return;
    const int f = fio_fmt(fmt, b);
    const bool valid = f >= 0 && offset_dev[b] > (long)max_delay;
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (c == 0) {
        o.x = valid ? 1u : 0u;
        o.y = valid ? (unsigned)(int)tokens[(long)b * tok_stride] : 0xffffffffu;
        o.z = valid ? (unsigned)(f == 1 ? 2 * F : 4 * F) : 0u;
    } else if (valid) {
        const long row = (long)b * F;
        const float* w = wav + row;
        if (f == 1) {
            const int i0 = (c - 1) * 8;
            if (i0 < F) {
                float v[8];
                if (i0 + 7 < F && wide && ((row & 3) == 0)) {
                    const float4 a = *reinterpret_cast<const float4*>(w + i0), d = *reinterpret_cast<const float4*>(w + i0 + 4);
                    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = d.x; v[5] = d.y; v[6] = d.z; v[7] = d.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = fio_load(w, i0 + j, F);
                }
                unsigned h[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = i0 + j < F ? fio_s16(v[j]) : 0u;
                o = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            }
        } else {
            const int i0 = (c - 1) * 4;
            if (i0 < F) {
                if (i0 + 3 < F && wide && ((row & 3) == 0)) {
                    const float4 a = *reinterpret_cast<const float4*>(w + i0);
                    o = make_uint4(__float_as_uint(a.x), __float_as_uint(a.y), __float_as_uint(a.z), __float_as_uint(a.w));
                } else {
                    o.x = __float_as_uint(fio_load(w, i0, F));
                    o.y = i0 + 1 < F ? __float_as_uint(w[i0 + 1]) : 0u;
                    o.z = i0 + 2 < F ? __float_as_uint(w[i0 + 2]) : 0u;
                    o.w = i0 + 3 < F ? __float_as_uint(w[i0 + 3]) : 0u;
                }
            }
        }
    }
    *reinterpret_cast<uint4*>(out + (long)b * rec_stride + (long)c * 16) = o;
}

int fio_check(const char* what, const void* rec, const void* fmt, const void* pcm, int B, int F, long rec_stride) {
    RST_REQUIRE(B >= 0 && B <= 65535 && F >= 1 && F <= (1 << 24), "%s: B in [0, 65535] and F in [1, 2^24] required (B=%d F=%d)", what, B, F);
    const long need = (16 + 4 * (long)F + 15) / 16 * 16;
    RST_REQUIRE(rec_stride >= need && rec_stride % 16 == 0 && rec_stride <= (1L << 30),
                "%s: the record stride must be a multiple of 16, at least round_up(16 + 4 F, 16) = %ld and at most 2^30 (got %ld)", what, need,
                rec_stride);
    if (B == 0) return RST_OK;
    RST_REQUIRE(rec && fmt && pcm, "%s: null pointer", what);
    RST_REQUIRE(((uintptr_t)rec & 15) == 0 && ((uintptr_t)pcm & 3) == 0 && ((uintptr_t)fmt & 3) == 0,
                "%s: the record buffer must be 16-byte aligned, the fp32 frame and fmt 4-byte aligned", what);
    return RST_OK;
}

// the fp32 side may move float4 only from a 16-byte-aligned base (a view into a larger tensor need not be)
int fio_wide(const void* pcm) { return ((uintptr_t)pcm & 15) == 0; }

}  // namespace

int rst_launch_frame_ingress(const unsigned char* staged, const int* fmt, float* pcm_out, int B, int F, long rec_stride, hipStream_t stream) {
    const int rc = fio_check("frame_ingress", staged, fmt, pcm_out, B, F, rec_stride);
    if (rc != RST_OK || B == 0) return rc;
    const int quads = (F + 3) / 4;
    hipLaunchKernelGGL(frame_ingress_kernel, dim3((quads + FIO_THREADS - 1) / FIO_THREADS, B), dim3(FIO_THREADS), 0, stream, staged, fmt,
                       pcm_out, F, rec_stride, fio_wide(pcm_out));
    return rst_check_launch("frame_ingress");
}

int rst_launch_frame_egress(const float* wav, const long* tokens, int tok_stride, const long* offset_dev, int max_delay, const int* fmt,
                            unsigned char* out, int B, int F, long rec_stride, hipStream_t stream) {
    const int rc = fio_check("frame_egress", out, fmt, wav, B, F, rec_stride);
    if (rc != RST_OK || B == 0) return rc;
    RST_REQUIRE(tokens && offset_dev && tok_stride >= 1 && max_delay >= 0,
                "frame_egress: tokens, offset_dev, tok_stride >= 1 and max_delay >= 0 required (tok_stride=%d max_delay=%d)", tok_stride, max_delay);
    RST_REQUIRE(((uintptr_t)tokens & 7) == 0 && ((uintptr_t)offset_dev & 7) == 0, "frame_egress: tokens and offset_dev are int64 (8-byte aligned)");
    const int chunks = (int)(rec_stride / 16);
    hipLaunchKernelGGL(frame_egress_kernel, dim3((chunks + FIO_THREADS - 1) / FIO_THREADS, B), dim3(FIO_THREADS), 0, stream, wav, tokens,
                       tok_stride, offset_dev, max_delay, fmt, out, F, rec_stride, fio_wide(wav));
    return rst_check_launch("frame_egress");
}
